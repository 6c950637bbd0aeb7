"""Forced playouts and policy-target pruning without a GPU: the library's host export
(gz_puct_forced_prune_host, the lines of csrc/gz_forced.h the device runs) against the
plain-Python restatement tests/puct_forced_ref.py, the reference's own behaviour on a
synthetic evaluator, the argument checks of gzero.device.puct_params, and the header alone
in a host program under the sanitizers."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import puct_forced_ref as FR
import puct_ref as R
from conftest import REPO
from gzero import _lib, device

C_PUCT = 1.6
CELLS = 225


def _host(k, N, prior, W, visits, c_puct=C_PUCT):
    return [int(x) for x in device.forced_prune_host(c_puct, k, N, prior, W, visits)]


# ---------------------------------------------------------------- 1. the host export
def _random_row(rng, dense):
    visits = np.where(rng.random(CELLS) < dense, rng.integers(0, 61, CELLS), 0).astype(np.int32)
    prior = rng.dirichlet(np.full(CELLS, 0.3 if rng.random() < 0.5 else 0.03))
    W = rng.uniform(-1.0, 1.0, CELLS) * visits
    return prior, W, visits


def test_host_export_equals_the_reference_on_random_rows():
    rng = np.random.default_rng(5)
    seen = dict(pruned=0, to_zero=0, capped_by_n=0, unchanged=0, ties=0)
    for i in range(2000):
        prior, W, visits = _random_row(rng, (0.05, 0.3, 0.9)[i % 3])
        k = (0.0, 0.5, 2.0, 2.0, 16.0)[i % 5]
        if i % 7 == 0 and visits.max() > 0:  # c* ties: a second cell with the most visits, before or after it
            first = int(np.argmax(visits))
            other = (first + (37 if i % 2 else 188)) % CELLS
            visits[other] = visits[first]
            W[other] = W[first] * 0.5
            seen["ties"] += 1
        N = int(visits.sum()) + 1 + int(rng.integers(0, 3))
        want = FR.prune_counts(C_PUCT, k, N, [float(x) for x in prior], [float(x) for x in W], [int(x) for x in visits])
        got = _host(k, N, prior, W, visits)
        assert got == want, i
        assert sum(got) <= int(visits.sum()) and (sum(got) > 0) == (visits.max() > 0)
        if k == 0.0:
            assert got == [int(x) for x in visits]
        best = int(np.argmax(visits))
        assert got[best] == visits[best]
        for c in np.flatnonzero(visits):
            n, out = int(visits[c]), got[c]
            seen["pruned"] += out < n
            seen["to_zero"] += out == 0 and n >= 2  # n - r == 1 gives 0
            seen["capped_by_n"] += FR.forced_min(k, float(prior[c]), N - 1) > n
            seen["unchanged"] += out == n
    print(seen)
    assert all(v > 0 for v in seen.values()), seen


def test_host_export_edge_rows():
    prior = np.full(CELLS, 1.0 / CELLS)
    W = np.zeros(CELLS)
    # no child: the row is unchanged
    visits = np.zeros(CELLS, np.int32)
    assert _host(2.0, 1, prior, W, visits) == [0] * CELLS
    # a single child keeps its count
    visits[100] = 9
    assert _host(2.0, 10, prior, W, visits) == [int(x) for x in visits]
    # n - r == 1 becomes 0: a hopeless child (q = -1) with a large prior next to a good one
    prior = np.full(CELLS, 0.8 / 224)
    prior[7] = 0.2
    visits = np.zeros(CELLS, np.int32)
    visits[3], visits[7] = 30, 6
    W = np.zeros(CELLS)
    W[3], W[7] = 15.0, -6.0
    # k = 2: (int)sqrt(2 * 0.2 * 36) = 3 visits may come off, and do (best is about 0.5; the cell
    # scores -1 + 1.95 / (1 + count) < 0.5 down to count 3)
    want = FR.prune_counts(C_PUCT, 2.0, 37, list(map(float, prior)), list(map(float, W)), list(map(int, visits)))
    assert _host(2.0, 37, prior, W, visits) == want and want[7] == 3 and want[3] == 30
    # a forced threshold above n (sqrt(16 * 0.2 * 36) > 10 > 6): at most n come off; here five do
    # (with no visit the cell scores -1 + 1.95 >= best), and n - r == 1 becomes 0
    assert FR.forced_min(16.0, 0.2, 36) > 6
    want = FR.prune_counts(C_PUCT, 16.0, 37, list(map(float, prior)), list(map(float, W)), list(map(int, visits)))
    assert _host(16.0, 37, prior, W, visits) == want and want[7] == 0 and sum(want) == 30
    # the arguments
    L = _lib.load()
    out = np.zeros(CELLS, np.int32)
    for k in (float("nan"), -1.0, 17.0, float("inf")):
        assert L.gz_puct_forced_prune_host(C_PUCT, k, 37, prior.ctypes.data, W.ctypes.data, visits.ctypes.data,
                                           out.ctypes.data) == -1  # GZ_ERR_ARG
    assert L.gz_puct_forced_prune_host(C_PUCT, 2.0, 0, prior.ctypes.data, W.ctypes.data, visits.ctypes.data,
                                       out.ctypes.data) == -1  # GZ_ERR_ARG
    assert not out.any()


def test_new_symbols_and_struct():
    L = _lib.load()
    hdr = open(os.path.join(REPO, "include", "gzero.h")).read()
    assert "#define GZ_PUCT_FORCED_PLAYOUTS 16" in hdr and _lib.GZ_PUCT_FORCED_PLAYOUTS == 16
    assert ("int gz_puct_forced_prune_host(double c_puct, double forced_k, int32_t root_visits, "
            "const double prior[225],") in hdr
    assert hasattr(L, "gz_puct_forced_prune_host")
    import ctypes
    assert ctypes.sizeof(_lib.PuctForcedParams) == 80 and _lib.PuctForcedParams.forced_k.offset == 72


# ---------------------------------------------------------------- 2. the reference on a synthetic evaluator
X = 112  # the cell with prior 0.5 that loses for whoever plays it
Y = 96   # the cell with prior 0.3 that is good for whoever plays it


def peaked_eval(cells, player):
    """Prior 0.5 on X, 0.3 on Y, the rest uniform over the other empty cells; every position
    with a stone on X is lost for the stone's owner (so the move is worth -1 to its mover and
    every backup through it says so), else one with a stone on Y is worth 0.5 to that stone's
    owner, and every other position is even."""
    rest = [c for c in range(CELLS) if cells[c] == 0 and c not in (X, Y)]
    prior = [0.0] * CELLS
    left = 1.0
    for c, p in ((X, 0.5), (Y, 0.3)):
        if cells[c] == 0:
            prior[c] = p
            left -= p
    for c in rest:
        prior[c] = left / len(rest)
    if cells[X] != 0:
        return prior, (1.0 if player != cells[X] else -1.0)
    if cells[Y] != 0:
        return prior, (-0.5 if player != cells[Y] else 0.5)
    return prior, 0.0


def _fields(t):
    return (t.parent, t.move, t.term, t.visits, t.W, t.child, t.prior, t.value, t.cells, t.player, t.count)


def test_reference_forces_the_peaked_cell_and_prunes_it_again():
    S, k = 40, 2.0
    cnt = FR.Counters()
    t = FR.search([0] * CELLS, 1, 0, S, C_PUCT, peaked_eval, k, counters=cnt)
    plain = R.search([0] * CELLS, 1, 0, S, C_PUCT, peaked_eval)
    j = t.child[0][X]
    n, n_plain = t.visits[j], plain.visits[plain.child[0][X]]
    print(f"visits of X: forced {n}, plain {n_plain}; threshold {FR.forced_min(k, 0.5, S - 1):.3f}; "
          f"forced selections {cnt.forced_selections}")
    assert t.W[j] == -float(n)
    # revisited until n >= forced (the threshold of the last simulation, T = S - 1)
    assert float(n) >= FR.forced_min(k, t.prior[0][X], S - 1) and n > n_plain and cnt.forced_selections >= 1
    before = [list(x) if isinstance(x, list) else x for x in _fields(t)]
    move = R.choose_move(t, 0, 1, 0)
    row = FR.prune_row(t, C_PUCT, k, cnt)
    # the tree and the move are those of the same search without pruning
    assert [list(x) if isinstance(x, list) else x for x in _fields(t)] == before
    assert R.choose_move(t, 0, 1, 0) == move and move[0] != X
    raw = t.root_visits()
    print(f"row at X: raw {raw[X]}, pruned {row[X]}; pruned visits {cnt.pruned_visits}")
    assert cnt.pruned_visits == sum(raw) - sum(row) >= 1
    # 0, or no more than PUCT alone gave the cell
    assert row[X] == 0 or row[X] <= n_plain
    # what is left was earned: with one visit fewer the cell would score at least the best child's score
    best_c = max(range(CELLS), key=lambda c: (raw[c], -c))
    sq = math.sqrt(float(t.visits[0]))
    bj = t.child[0][best_c]
    best = t.W[bj] / raw[best_c] + ((C_PUCT * t.prior[0][best_c]) * sq) / (1.0 + raw[best_c])
    for c, jj in t.child[0].items():
        if c != best_c and 1 < row[c] < raw[c]:
            q = t.W[jj] / raw[c]
            assert q + ((C_PUCT * t.prior[0][c]) * sq) / (1.0 + (row[c] - 1)) >= best, c
    assert sum(row) > 0 and row[best_c] == raw[best_c]


def test_k_zero_is_puct_ref_byte_for_byte():
    cells, player, n_moves = R.tactical_position()
    for ev in (R.uniform_eval, peaked_eval):
        cnt = FR.Counters()
        a = FR.search(cells, player, n_moves, 48, C_PUCT, ev, 0.0, counters=cnt)
        b = R.search(cells, player, n_moves, 48, C_PUCT, ev)
        assert _fields(a) == _fields(b)
        assert FR.prune_row(a, C_PUCT, 0.0, cnt) == b.root_visits()
        assert cnt.forced_selections == 0 and cnt.pruned_visits == 0
    moves_a = FR.play_game(3, 0, 12, C_PUCT, 2, R.uniform_eval, 0.0, max_plies=6)
    import puct_reuse_ref as RR
    moves_b = RR.play_game(3, 0, 12, C_PUCT, 2, R.uniform_eval, max_plies=6)
    assert moves_a[0] == moves_b[0] and moves_a[1] == moves_b[1] == moves_a[2]


# ---------------------------------------------------------------- 3. puct_params
def test_puct_params_builds_the_struct_and_rejects_bad_arguments():
    p = device.puct_params(40, C_PUCT, 2, 9, "f16x3", forced_playouts=2.0)
    assert isinstance(p, _lib.PuctForcedParams) and p.flags == _lib.GZ_PUCT_FORCED_PLAYOUTS and p.forced_k == 2.0
    assert (p.num_simulations, p.temp_plies, p.c_puct, p.seed) == (40, 2, C_PUCT, 9)
    p = device.puct_params(40, C_PUCT, 2, 9, "fp32", dirichlet_alpha=0.3, noise_eps=0.25, fast_simulations=8,
                           full_prob=0.5, leaf_symmetry=True, forced_playouts=0.0)
    assert p.flags == (_lib.GZ_PUCT_ROOT_NOISE | _lib.GZ_PUCT_PLAYOUT_CAP | _lib.GZ_PUCT_LEAF_SYM |
                       _lib.GZ_PUCT_FORCED_PLAYOUTS)
    assert (p.noise_alpha, p.noise_eps, p.fast_simulations, p.full_prob, p.forced_k) == (0.3, 0.25, 8, 0.5, 0.0)
    # None leaves the flag clear and the struct as it was
    q = device.puct_params(40, C_PUCT, 2, 9, "f16x3")
    assert type(q) is _lib.PuctParams and q.flags == 0
    for bad in (float("nan"), -1.0, 17.0, float("inf")):
        with pytest.raises(ValueError, match="forced_playouts must be in"):
            device.puct_params(40, forced_playouts=bad)
    with pytest.raises(ValueError, match="forced_playouts is not supported with leaves_per_round > 1"):
        device.puct_params(40, leaves_per_round=4, forced_playouts=2.0)
    with pytest.raises(ValueError, match="leaves_per_round > 1 is not supported with forced_playouts"):
        device.with_leaves(device.puct_params(40, forced_playouts=2.0), 4)


def _rejected(p, word):
    """Every entry point that takes the params returns GZ_ERR_ARG and names the cause (the
    checks come before every GPU call: any non-NULL pointer will do)."""
    import ctypes
    L = _lib.load()
    pp = ctypes.cast(ctypes.pointer(p), ctypes.POINTER(_lib.PuctParams))
    one = ctypes.c_int64(0)
    ptr = ctypes.addressof(one)
    calls = (lambda: L.gz_puct_search(ptr, ptr, 1, pp, ptr, ptr, ptr, ptr, ptr, None),
             lambda: L.gz_puct_begin(ptr, ptr, 1, pp, ptr, ptr, ptr, None),
             lambda: L.gz_selfplay_puct_run(ptr, 1, pp, ptr, ptr, 1, ptr, 0, ptr, ptr, None),
             lambda: L.gz_selfplay_puct_run_active(ptr, 1, 1, pp, ptr, ptr, 1, ptr, 0, ptr, ptr, None),
             lambda: L.gz_selfplay_puct_rounds(ptr, 1, pp, ptr, ptr, 1, ptr, 0, ptr, ptr, None),
             lambda: L.gz_selfplay_puct_rounds_active(ptr, 1, 1, pp, ptr, ptr, 1, ptr, 0, ptr, ptr, None))
    for call in calls:
        assert call() == -1 and word in L.gz_last_error(), L.gz_last_error()


def _raw_params(k, flags=_lib.GZ_PUCT_FORCED_PLAYOUTS):
    return _lib.PuctForcedParams(8, 0, C_PUCT, 1, _lib.GZ_PV_F16X3, flags, 0.3, 0.25, 4, 0, 4, 0, 0.5, k)


@pytest.mark.parametrize("k", [float("nan"), -1.0, 17.0, float("inf")])
def test_forced_k_out_of_range_is_an_argument_error(k):
    _rejected(_raw_params(k), b"forced_k")


def test_the_flag_with_leaf_batching_or_in_a_match_is_an_argument_error():
    import ctypes
    _rejected(_raw_params(2.0, _lib.GZ_PUCT_FORCED_PLAYOUTS | _lib.GZ_PUCT_LEAF_BATCH), b"leaf batching")
    L = _lib.load()
    p = _raw_params(2.0)
    one = ctypes.c_int64(0)
    ptr = ctypes.addressof(one)
    mp = _lib.PuctMatchParams(ctypes.cast(ctypes.pointer(p), ctypes.c_void_p), (ctypes.c_void_p * 2)(ptr, ptr),
                              (ctypes.c_int32 * 2)(_lib.GZ_PV_F16X3, _lib.GZ_PV_F16X3), 0, 0)
    assert L.gz_puct_match_run(ptr, 1, 1, ctypes.byref(mp), ptr, 1, ptr, 0, ptr, ptr, None) == -1
    assert b"forced playouts" in L.gz_last_error()
    # without the flag nothing past the cap struct is read: a NaN there is not an error of its own
    q = _raw_params(float("nan"), 0)
    pp = ctypes.cast(ctypes.pointer(q), ctypes.POINTER(_lib.PuctParams))
    assert L.gz_puct_search(None, None, 1, pp, None, None, None, None, None, None) == -1
    assert b"forced_k" not in L.gz_last_error() and b"bad arguments" in L.gz_last_error()


# ---------------------------------------------------------------- 4. the header alone, under the sanitizers
def _recurrence_rows():
    """The rows tests/hosttest/forced_main.cpp prunes, by the same integer recurrence."""
    state = 20240917
    mask = (1 << 64) - 1

    def nxt():
        nonlocal state
        state = (state * 6364136223846793005 + 1442695040888963407) & mask
        return state >> 33

    rows = []
    n_rows = 48
    for row in range(n_rows):
        visits, prior, W = [0] * CELLS, [0.0] * CELLS, [0.0] * CELLS
        every = 2 if row % 3 == 0 else 8
        for c in range(CELLS):
            a, b, d, e = nxt(), nxt(), nxt(), nxt()
            visits[c] = 1 + b % 40 if a % every == 0 else 0
            prior[c] = float(1 + d % 1000) / 4096.0
            W[c] = (float(e % 2001 - 1000) / 1000.0) * float(visits[c])
        if row == 1:
            visits = [9 if c == 77 else 0 for c in range(CELLS)]
        if row == 2:
            visits = [0] * CELLS
        rows.append(((0.0, 1.0, 2.0, 16.0)[row % 4], sum(visits) + 1, prior, W, visits))
    return rows


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_forced_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "forced_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(REPO, "tests", "hosttest", "forced_main.cpp"),
                    "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, \
        (r.stdout[-2000:], r.stderr[-2000:])
    lines = [x for x in r.stdout.split("\n") if x.strip()]
    rows = _recurrence_rows()
    assert lines[-1] == "ok" and len(lines) == len(rows) + 1
    pruned = 0
    for i, (line, (k, N, prior, W, visits)) in enumerate(zip(lines, rows)):
        f = line.split()
        assert f[0] == "row" and int(f[1]) == i and float(f[2]) == k and int(f[3]) == N
        got = [int(x) for x in f[4:]]
        if i == len(rows) - 1:
            # the NaN prior sits at the least-visited child: nothing is forced there, its count stays
            worst = min((c for c in range(CELLS) if visits[c] > 0), key=lambda c: (visits[c], c))
            prior = list(prior)
            prior[worst] = 0.0
            assert got[worst] == visits[worst]
        assert got == FR.prune_counts(C_PUCT, k, N, prior, W, visits), i
        pruned += sum(visits) - sum(got)
    assert pruned > 0
