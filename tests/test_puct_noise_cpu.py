"""The Dirichlet root noise of the PUCT search without a GPU: the host build of the
sampler (gz_puct_root_noise_host, the GZ_HD code of csrc/gz_dirichlet.h) against the
plain-Python restatement in tests/puct_noise_ref.py bit for bit, the accuracy of the
plain-arithmetic log / exp, the distribution of eta, and the library / Python surface."""
import ctypes
import math
import random

import numpy as np
import pytest

import puct_noise_ref as NR
from gzero import _lib, device

ULP4 = 4 * 2.0 ** -52  # 8.9e-16


def _mid_game():
    """87 stones scattered by a fixed rule."""
    return [(c * 37 + 11) % 225 % 13 >= 5 for c in range(225)]


EMPTY = [True] * 225
ONE = [c == 100 for c in range(225)]


# ---------------------------------------------------------------- (a) host == reference
@pytest.mark.parametrize("alpha", [0.03, 0.3, 1.0, 2.5])
def test_host_sampler_equals_the_reference_bitwise(alpha):
    mid = _mid_game()
    assert 100 < sum(mid) < 200
    for empty in (EMPTY, ONE, mid):
        for gid in (0, (1 << 40) + 3):
            for ply in (0, 7, 199):
                got = device.puct_root_noise_host(7, gid, ply, empty, alpha)
                ref = NR.eta_row(7, gid, ply, empty, alpha)
                assert [float(x) for x in got] == ref, (gid, ply)  # float64, bit for bit
                assert all(x == 0.0 for x, e in zip(got, empty) if not e)
                if empty is ONE:
                    assert got[100] == 1.0
    # and a row that does not depend on which other cells are empty only through the total
    a = device.puct_root_noise_host(7, 5, 3, EMPTY, alpha)
    b = device.puct_root_noise_host(7, 5, 3, mid, alpha)
    i, j = [c for c in range(225) if mid[c]][:2]
    assert a[i] > 0 and b[i] > 0 and abs(a[i] / a[j] - b[i] / b[j]) <= 1e-12 * (a[i] / a[j])


def test_a_full_board_gives_a_zero_row():
    got = device.puct_root_noise_host(1, 2, 3, [False] * 225, 0.3)
    assert not got.any() and NR.eta(1, 2, 3, [False] * 225, 0.3) is None


# ---------------------------------------------------------------- (b) accuracy
def test_log_and_exp_are_within_four_ulp():
    r = random.Random(20250)
    worst_log = worst_exp = 0.0
    for _ in range(200000):
        x = math.ldexp(r.uniform(0.5, 1.0), r.randint(-60, 3))
        want = math.log(x)
        if want != 0.0:
            worst_log = max(worst_log, abs(NR.gz_log(x) - want) / abs(want))
        y = r.uniform(-700.0, 0.0)
        want = math.exp(y)
        worst_exp = max(worst_exp, abs(NR.gz_exp(y) - want) / want)
    print(f"largest relative error: gz_log {worst_log:.3e}, gz_exp {worst_exp:.3e} (bound {ULP4:.3e})")
    assert worst_log <= ULP4 and worst_exp <= ULP4
    assert NR.gz_log(1.0) == 0.0 and NR.gz_exp(0.0) == 1.0 and NR.gz_exp(-708.5) == 0.0
    assert NR.unit(0) == 2.0 ** -53 and NR.unit((1 << 64) - 1) == 1.0


# ---------------------------------------------------------------- (c) distribution
@pytest.mark.parametrize("alpha", [0.3, 0.03, 1.0])
def test_eta_has_the_dirichlet_mean_and_variance(alpha):
    L = 225
    rows = np.array([device.puct_root_noise_host(7, gid, 3, EMPTY, alpha) for gid in range(400)])
    assert rows.shape == (400, L) and (rows >= 0).all()
    assert np.abs(rows.sum(axis=1) - 1.0).max() < 1e-12
    assert abs(rows.mean() - 1.0 / L) < 1e-15 * L
    want = (1.0 / L) * (1.0 - 1.0 / L) / (L * alpha + 1.0)
    ratio = rows.var() / want
    print(f"alpha {alpha}: variance / Dirichlet variance = {ratio:.3f}")
    assert 0.9 <= ratio <= 1.1
    if alpha == 0.3:  # the draws a cell uses stay far inside the 256 it owns
        used = []
        key = NR.noise_key(7, 0, 3)
        for c in range(225):
            NR.gamma_cell(key, c, alpha, used)
        assert max(used) < 64


# ---------------------------------------------------------------- (d) surface
def test_library_has_the_noise_entry_points():
    L = _lib.load()
    for name in ("gz_puct_root_noise", "gz_puct_root_noise_host"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert ctypes.sizeof(_lib.PuctParams) == 32 and ctypes.sizeof(_lib.PuctNoiseParams) == 48
    assert _lib.PuctNoiseParams.noise_alpha.offset == 32 and _lib.PuctNoiseParams.noise_eps.offset == 40
    assert _lib.GZ_PUCT_ROOT_NOISE == 1
    p = device.puct_params(16, 1.6, 0, 3, dirichlet_alpha=0.3)
    assert isinstance(p, _lib.PuctNoiseParams) and p.flags == 1 and p.noise_alpha == 0.3 and p.noise_eps == 0.25
    q = device.puct_params(16, 1.6, 0, 3)
    assert type(q) is _lib.PuctParams and q.flags == 0
    assert bytes(q) == bytes(p)[:28] + b"\0\0\0\0"  # the same base but for the flag


@pytest.mark.parametrize("alpha,eps,bad", [(float("nan"), 0.25, True), (float("inf"), 0.25, True), (0.0, 0.25, True),
                                            (5e-4, 0.25, True), (1001.0, 0.25, True), (-0.3, 0.25, True),
                                            (0.3, -0.01, True), (0.3, 1.01, True), (0.3, float("nan"), True),
                                            (1e-3, 0.0, False), (1e3, 1.0, False)])
def test_library_rejects_bad_noise(alpha, eps, bad):
    L = _lib.load()
    p = _lib.PuctNoiseParams(16, 0, 1.6, 0, _lib.GZ_PV_F16X3, _lib.GZ_PUCT_ROOT_NOISE, alpha, eps)
    calls = {
        "gz_puct_search": lambda: L.gz_puct_search(None, None, 1, ctypes.byref(p), None, None, None, None, None, None),
        "gz_puct_begin": lambda: L.gz_puct_begin(None, None, 1, ctypes.byref(p), None, None, None, None),
        "gz_selfplay_puct_run": lambda: L.gz_selfplay_puct_run(None, 1, ctypes.byref(p), None, None, 1, None, 0, None,
                                                               None, None),
        "gz_selfplay_puct_rounds": lambda: L.gz_selfplay_puct_rounds(None, 1, ctypes.byref(p), None, None, 1, None, 0,
                                                                     None, None, None),
    }
    for name, call in calls.items():
        assert call() == -1, name  # (NULL pointers: an error either way)
        assert (b"noise" in L.gz_last_error()) == bad, (name, L.gz_last_error())
    if bad and not 1e-3 <= alpha <= 1e3:
        out = (ctypes.c_double * 225)()
        e = (ctypes.c_uint8 * 225)(*([1] * 225))
        assert L.gz_puct_root_noise_host(1, 0, 0, e, alpha, out) == -1 and b"noise" in L.gz_last_error()
        assert L.gz_puct_root_noise(None, None, 0, 1, alpha, None, None) == -1 and b"noise" in L.gz_last_error()
    # with the flag clear the same bytes are not looked at
    p.flags = 0
    assert L.gz_puct_search(None, None, 1, ctypes.byref(p), None, None, None, None, None, None) == -1
    assert b"noise" not in L.gz_last_error()


def test_python_value_errors():
    import training
    from gzero.selfplay import SelfPlayEngine
    with pytest.raises(ValueError, match="dirichlet_alpha"):
        SelfPlayEngine(n_slots=8, dirichlet_alpha=0.3)  # the default search
    with pytest.raises(ValueError, match="dirichlet_alpha"):
        SelfPlayEngine(n_slots=8, search="reference", dirichlet_alpha=0.3, noise_eps=0.5)
    with pytest.raises(ValueError, match="dirichlet_alpha"):
        training.run_iteration(None, None, 1, search="reference", dirichlet_alpha=0.3)
    for alpha in (0.0, 1e4, float("nan"), -1.0):
        with pytest.raises(ValueError, match="dirichlet_alpha"):
            device.puct_params(16, dirichlet_alpha=alpha)
    for eps in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="noise_eps"):
            device.puct_params(16, dirichlet_alpha=0.3, noise_eps=eps)
    with pytest.raises(ValueError):
        device.puct_root_noise_host(0, 0, 0, [True] * 224, 0.3)


# ---------------------------------------------------------------- (e) the reference's wrappers
def test_reference_mixes_each_root_once():
    import puct_ref as R
    import puct_reuse_ref as RR
    noise = NR.Noise(3, 11, 0.3, 0.25)
    cells, player, n_moves = R.tactical_position()
    t = NR.search(cells, player, n_moves, 24, 1.6, R.uniform_eval, noise)
    plain = R.search(cells, player, n_moves, 24, 1.6, R.uniform_eval)
    want = NR.mix(plain.prior[0], cells, 3, 11, n_moves, 0.3, 0.25)
    assert t.prior[0] == want and t.prior[0] != plain.prior[0]
    assert abs(sum(t.prior[0]) - 1.0) < 1e-12
    for k in range(1, len(t.parent)):  # other nodes keep the evaluator's rows
        if t.term[k] == 0:
            assert t.prior[k] == R.uniform_eval(list(t.cells[k]), t.player[k])[0]
    mv = max((c for c, k in t.child[0].items() if t.term[k] == 0), key=lambda c: t.root_visits()[c])
    j = t.child[0][mv]
    carried = list(t.prior[j])
    nt, over = NR.advance(t, mv, noise)
    assert not over and nt.prior[0] == NR.mix(carried, nt.cells[0], 3, 11, n_moves + 1, 0.3, 0.25)
    assert t.prior[j] == carried  # the old tree's row is not the one mixed
    # a move without a child: a fresh root that is mixed at its evaluation
    cold = next(c for c in range(225) if cells[c] == 0 and c not in t.child[0])
    ft, over = NR.advance(t, cold, noise)
    assert not over and ft.prior[0] is None
    NR.evaluate(ft, R.uniform_eval, noise)
    assert ft.prior[0] == NR.mix(R.uniform_eval(list(ft.cells[0]), 0)[0], ft.cells[0], 3, 11, n_moves + 1, 0.3, 0.25)
    # eps 0: the mix is the identity
    zero = NR.search(cells, player, n_moves, 24, 1.6, R.uniform_eval, NR.Noise(3, 11, 0.3, 0.0))
    assert zero.prior == plain.prior and zero.visits == plain.visits and zero.W == plain.W
    assert RR.CELLS == 225
