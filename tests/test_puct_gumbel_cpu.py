"""The Gumbel root with sequential halving without a GPU: the library's host exports
(gz_puct_gumbel_sequence_host, gz_puct_gumbel_root_host, gz_puct_gumbel_policy_host -- the
lines of csrc/gz_gumbel.h the device runs) against the plain-Python restatement
tests/puct_gumbel_ref.py, the sampler's distribution, the restatement's own behaviour on
synthetic evaluators, the struct and the argument checks, and the header alone in a host
program under the sanitizers."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import puct_gumbel_ref as GR
import puct_ref as R
from conftest import REPO
from gzero import _lib, device

C_PUCT = 1.6
CELLS = 225
NEG_INF = -math.inf


def _bits(xs):
    return np.asarray(xs, np.float64).view(np.uint64).tolist()


# ---------------------------------------------------------------- 1. the schedule
def test_sequence_equals_the_reference_and_the_issue_examples():
    assert GR.seq(16, 32) == [0] * 16 + [1] * 8 + [2] * 4 + [3] * 4
    assert GR.seq(4, 8) == [0, 0, 0, 0, 1, 1, 2, 2]
    for m in range(1, 33):
        for S in (1, 2, 5, 16, 32, 33, 200, 4095):
            got = device.puct_gumbel_sequence_host(m, S).tolist()
            assert got == GR.seq(m, S), (m, S)
            assert len(got) == S and got[0] == 0
    L = _lib.load()
    buf = (ctypes.c_int16 * 8)()
    for m, S in ((0, 8), (33, 8), (4, 0), (4, 4096)):
        assert L.gz_puct_gumbel_sequence_host(m, S, ctypes.addressof(buf)) == -1
    assert L.gz_puct_gumbel_sequence_host(4, 8, None) == -1


# ---------------------------------------------------------------- 2. the root preparation
def _root_both(seed, gid, ply, prior, empty, mc, scale):
    got = device.puct_gumbel_root_host(seed, gid, ply, prior, empty, mc, scale)
    want, taken = GR.root(seed, gid, ply, [float(x) for x in prior], [bool(x) for x in empty], mc, scale)
    assert _bits(got) == _bits(want), (seed, gid, ply, mc, scale)
    return got, taken


def test_root_host_equals_the_reference_on_random_rows():
    rng = np.random.default_rng(11)
    for i in range(120):
        empty = rng.random(CELLS) < (0.95, 0.5, 0.1)[i % 3]
        empty[int(rng.integers(CELLS))] = True
        prior = rng.dirichlet(np.full(CELLS, 0.3 if i % 2 else 0.03))
        mc = (1, 2, 3, 16, 32)[i % 5]
        gs, taken = _root_both(5 + i, 100 + i, i % 200, prior, empty, mc, (1.0, 0.0, 2.5)[i % 3])
        ok = empty & (prior >= GR.DBL_MIN)
        n_ok = int(ok.sum()) if ok.any() else int(empty.sum())
        assert len(taken) == min(mc, n_ok) == int(np.isfinite(gs).sum())
        assert all(empty[c] for c in taken) and np.all(gs[~np.isfinite(gs)] == NEG_INF)


def test_root_host_on_zeros_denormals_a_nan_three_cells_and_no_ok_cell():
    rng = np.random.default_rng(12)
    prior = rng.dirichlet(np.full(CELLS, 0.3))
    empty = np.ones(CELLS, bool)
    empty[::7] = False
    prior[1::7] = 0.0
    prior[2], prior[3], prior[4], prior[5] = 5e-324, 1e-310, float("nan"), float("inf")
    gs, taken = _root_both(1, 2, 3, prior, empty, 32, 1.0)
    assert len(taken) == 32 and not set(taken) & {2, 3, 4, 5} and not any(c % 7 in (0, 1) for c in taken)
    # three empty cells: m becomes 3
    empty = np.zeros(CELLS, bool)
    empty[[7, 100, 224]] = True
    gs, taken = _root_both(1, 2, 3, rng.dirichlet(np.full(CELLS, 0.3)), empty, 16, 1.0)
    assert sorted(taken) == [7, 100, 224] and int(np.isfinite(gs).sum()) == 3
    # no ok cell: every empty cell is ok with logit 0.0, so gs is the Gumbel alone
    prior = np.where(np.arange(CELLS) % 2 == 0, 0.0, float("nan"))
    empty = np.arange(CELLS) % 3 != 0
    gs, taken = _root_both(9, 8, 7, prior, empty, 16, 1.0)
    key = GR.gumbel_key(9, 8, 7)
    assert len(taken) == 16 and all(gs[c] == GR.gumbel(key, c, 1.0) for c in taken) and all(empty[c] for c in taken)
    L = _lib.load()
    buf = np.zeros(CELLS)
    e8 = np.ones(CELLS, np.uint8)
    for mc, sc in ((0, 1.0), (33, 1.0), (16, -0.5), (16, 9.0), (16, float("nan"))):
        assert L.gz_puct_gumbel_root_host(1, 2, 3, buf.ctypes.data, e8.ctypes.data, mc, sc, buf.ctypes.data) == -1


# ---------------------------------------------------------------- 3. the policy target
def _policy_both(prior, W, visits, v0, cv=50.0, cs=0.5):
    pi, row = device.puct_gumbel_policy_host(prior, W, visits, v0, cv, cs)
    wpi, wrow = GR.policy([float(x) for x in prior], [True] * CELLS, [float(x) for x in W], [int(x) for x in visits],
                          float(v0), cv, cs)
    assert _bits(pi) == _bits(wpi) and row.tolist() == wrow
    stones = np.asarray(prior) == 0.0
    assert row.max() >= 146 and np.all(row[stones] == 0) and np.all(pi[stones] == 0.0) and row.max() <= 32767
    assert abs(math.fsum(pi.tolist()) - 1.0) <= 1e-12
    return pi, row


def _random_policy_row(rng, n_stones, n_children):
    prior = rng.dirichlet(np.full(CELLS, 0.3))
    stones = rng.choice(CELLS, n_stones, replace=False)
    prior[stones] = 0.0  # (the host export: a stone carries a prior that is not ok)
    free = np.flatnonzero(prior > 0.0)
    visits = np.zeros(CELLS, np.int32)
    kids = rng.choice(free, min(n_children, len(free)), replace=False)
    visits[kids] = rng.integers(1, 9, len(kids))
    W = rng.uniform(-1.0, 1.0, CELLS) * visits
    return prior, W, visits


def test_policy_host_equals_the_reference():
    rng = np.random.default_rng(13)
    for i in range(150):
        prior, W, visits = _random_policy_row(rng, (0, 40, 200)[i % 3], (1, 4, 16, 32)[i % 4])
        _policy_both(prior, W, visits, float(np.float32(rng.uniform(-1, 1))), (50.0, 0.0, 1e4)[i % 3], (0.5, 0.0, 3.0)[i % 3])
    # a single visited child
    prior, W, visits = _random_policy_row(rng, 30, 1)
    _policy_both(prior, W, visits, 0.25)
    # no visited child: pi = softmax of the logits = the prior over its ok cells, to rounding
    prior, W, visits = _random_policy_row(rng, 30, 0)
    pi, row = _policy_both(prior, W, visits, -0.5)
    assert np.abs(pi - prior / prior.sum()).max() < 1e-13
    # c_scale = 0: sigma vanishes, the same
    prior, W, visits = _random_policy_row(rng, 30, 16)
    pi, row = _policy_both(prior, W, visits, 0.3, 50.0, 0.0)
    assert np.abs(pi - prior / prior.sum()).max() < 1e-13
    L = _lib.load()
    buf = np.zeros(CELLS)
    iv = np.zeros(CELLS, np.int32)
    for cv, cs in ((-1.0, 0.5), (2e4, 0.5), (50.0, -1.0), (50.0, 2e3), (float("nan"), 0.5), (50.0, float("inf"))):
        assert L.gz_puct_gumbel_policy_host(buf.ctypes.data, buf.ctypes.data, iv.ctypes.data, 0.0, cv, cs,
                                            buf.ctypes.data, iv.ctypes.data) == -1
    iv[3] = -1
    assert L.gz_puct_gumbel_policy_host(buf.ctypes.data, buf.ctypes.data, iv.ctypes.data, 0.0, 50.0, 0.5,
                                        buf.ctypes.data, None) == -1


# ---------------------------------------------------------------- 4. the sampler samples the prior
def test_the_argmax_of_g_plus_logit_is_distributed_as_the_prior():
    cells, probs = (3, 64, 100, 128, 224), (0.5, 0.25, 0.125, 0.0625, 0.0625)
    prior, empty = [0.0] * CELLS, [False] * CELLS
    for c, p in zip(cells, probs):
        prior[c], empty[c] = p, True
    games = 20000
    count = dict.fromkeys(cells, 0)
    pr, em = np.asarray(prior), np.asarray(empty)
    for gid in range(games):
        gs = device.puct_gumbel_root_host(7, gid, 9, pr, em, 1, 1.0)
        count[int(np.argmax(gs))] += 1
        if gid % 997 == 0:  # the library's row is the restatement's: the arg-max of base
            base, ok = GR.base_row(7, gid, 9, prior, empty, 1.0)
            best = max((c for c in cells), key=lambda c: base[c])
            assert int(np.argmax(gs)) == best and gs[best] == base[best]
    for c, p in zip(cells, probs):
        se = math.sqrt(p * (1.0 - p) / games)
        print(f"cell {c}: frequency {count[c] / games:.5f}, prior {p}, {abs(count[c] / games - p) / se:.2f} standard errors")
        assert abs(count[c] / games - p) <= 3.0 * se, (c, count[c])


# ---------------------------------------------------------------- 5. the restatement's own behaviour
def peaked_eval(cells, player):
    """A favourite move (the first empty cell of a fixed order) and a value that depends on the
    position."""
    empty = [c for c in range(CELLS) if cells[c] == 0]
    w = {c: 1.0 + ((c * 37 + 11) % 17) for c in empty}
    w[empty[(len(empty) * 5) // 7]] = 60.0
    tot = sum(w.values())
    h = sum((i + 1) * x for i, x in enumerate(cells)) % 1000
    return [w[c] / tot if c in w else 0.0 for c in range(CELLS)], float(np.float32((h - 500) / 700.0))


def test_one_considered_move_without_noise_takes_every_simulation():
    cells, player, n_moves = R.tactical_position()
    gm = GR.Gumbel(3, 5, max_considered=1, gumbel_scale=0.0)
    t = GR.search(cells, player, n_moves, 12, C_PUCT, peaked_eval, gm)
    prior = t.prior[0]
    top = max((c for c in range(CELLS) if cells[c] == 0), key=lambda c: prior[c])
    assert t.considered == [top] and t.root_visits()[top] == 12 and sum(t.root_visits()) == 12
    assert GR.choose_move(t, gm) == top


@pytest.mark.parametrize("m,S,want", [(4, 8, [3, 3, 1, 1]), (16, 32, [4] * 4 + [2] * 4 + [1] * 8), (2, 5, [3, 2]),
                                      (3, 7, [3, 3, 1])])
def test_the_visit_counts_are_those_the_schedule_implies(m, S, want):
    gm = GR.Gumbel(3, 5, max_considered=m)
    t = GR.search([0] * CELLS, 1, 0, S, C_PUCT, peaked_eval, gm)
    v = t.root_visits()
    assert sorted((v[c] for c in t.considered), reverse=True) == want and sum(v) == S
    assert all(v[c] == 0 for c in range(CELLS) if c not in t.considered)
    # halving order: the cells that survive a phase are those with the best gs + sigma(q) then
    mv = GR.choose_move(t, gm)
    assert v[mv] == max(v) and mv in t.considered
    pi, row = GR.target(t, gm)
    assert max(row) >= 146 and abs(math.fsum(pi) - 1.0) <= 1e-12
    assert all(row[c] == 0 for c in range(CELLS) if t.cells[0][c] != 0)


def test_terminal_children_at_the_root_keep_the_schedule():
    cells, player, n_moves = R.tactical_position()
    gm = GR.Gumbel(1, 2, max_considered=16)
    t = GR.search(cells, player, n_moves, 33, C_PUCT, R.uniform_eval, gm)
    v = t.root_visits()
    # seq(16, 33): 16 x 0, 8 x 1, 4 x 2, 4 x 3, then one of the last two once more
    assert sorted((v[c] for c in t.considered), reverse=True) == [5, 4, 4, 4, 2, 2, 2, 2] + [1] * 8 and sum(v) == 33


# ---------------------------------------------------------------- 6. the struct, puct_params, the argument checks
def test_struct_layout_and_puct_params():
    P = _lib.PuctGumbelParams
    assert ctypes.sizeof(P) == 112 and _lib.GZ_PUCT_GUMBEL == 32 and _lib.GZ_PUCT_GUMBEL_MAX_CONSIDERED == 32
    assert (P.max_considered.offset, P.c_visit.offset, P.c_scale.offset, P.gumbel_scale.offset) == (80, 88, 96, 104)
    assert P.forced_k.offset == 72
    p = device.puct_params(32, C_PUCT, 2, 9, "f16x3", gumbel_considered=16)
    assert isinstance(p, P) and p.flags == _lib.GZ_PUCT_GUMBEL
    assert (p.max_considered, p.c_visit, p.c_scale, p.gumbel_scale) == (16, 50.0, 0.5, 1.0)
    assert (p.num_simulations, p.temp_plies, p.c_puct, p.seed, p.precision) == (32, 2, C_PUCT, 9, _lib.GZ_PV_F16X3)
    p = device.puct_params(16, precision="f16", leaf_symmetry=True, gumbel_considered=4, c_visit=0.0, c_scale=1.0,
                           gumbel_scale=0.0)
    assert p.flags == (_lib.GZ_PUCT_GUMBEL | _lib.GZ_PUCT_LEAF_SYM) and p.precision == _lib.GZ_PV_F16
    assert (p.max_considered, p.c_visit, p.c_scale, p.gumbel_scale) == (4, 0.0, 1.0, 0.0)
    q = device.puct_params(32, C_PUCT, 2, 9, "f16x3")
    assert type(q) is _lib.PuctParams and q.flags == 0
    for bad in (0, 33, -1):
        with pytest.raises(ValueError, match="gumbel_considered must be in"):
            device.puct_params(32, gumbel_considered=bad)
    for kw, word in ((dict(c_visit=-1.0), "c_visit"), (dict(c_visit=float("nan")), "c_visit"),
                     (dict(c_visit=1e5), "c_visit"), (dict(c_scale=-0.1), "c_scale"), (dict(c_scale=1e4), "c_scale"),
                     (dict(gumbel_scale=-1.0), "gumbel_scale"), (dict(gumbel_scale=8.5), "gumbel_scale"),
                     (dict(gumbel_scale=float("inf")), "gumbel_scale")):
        with pytest.raises(ValueError, match=word + " must be in"):
            device.puct_params(32, gumbel_considered=16, **kw)
    for kw in (dict(dirichlet_alpha=0.3), dict(leaves_per_round=4), dict(fast_simulations=8), dict(forced_playouts=2.0)):
        with pytest.raises(ValueError, match="gumbel_considered is not supported with"):
            device.puct_params(32, gumbel_considered=16, **kw)
    with pytest.raises(ValueError, match="leaves_per_round > 1 is not supported with gumbel_considered"):
        device.with_leaves(device.puct_params(32, gumbel_considered=16), 4)


def test_workspace_sizes():
    L = _lib.load()
    assert L.gz_puct_gumbel_bytes(1, 1, 1) == 2048 + 256
    assert L.gz_puct_gumbel_bytes(5, 16, 16) == 9216 + 512
    assert L.gz_puct_gumbel_bytes(4096, 200, 32) == 4096 * 1800 + 12800
    off = device.puct_params(16)
    on = device.puct_params(16, gumbel_considered=4)
    both = device.puct_params(16, gumbel_considered=4, leaf_symmetry=True)
    al = lambda x: (x + 255) & ~255
    fc = L.gz_puct_workspace_bytes(5, 16)
    assert device._puct_workspace_bytes(L, 5, off) == fc
    assert device._puct_workspace_bytes(L, 5, on) == al(fc) + L.gz_puct_gumbel_bytes(5, 16, 4)
    assert device._puct_workspace_bytes(L, 5, both) == al(fc + L.gz_puct_sym_bytes(5)) + L.gz_puct_gumbel_bytes(5, 16, 4)


def _raw(mc=16, cv=50.0, cs=0.5, gsc=1.0, flags=_lib.GZ_PUCT_GUMBEL, S=8):
    return _lib.PuctGumbelParams(S, 0, C_PUCT, 1, _lib.GZ_PV_F16X3, flags, 0.3, 0.25, 4, 0, 4, 0, 0.5, 2.0, mc, 0, cv, cs, gsc)


def _calls(p):
    L = _lib.load()
    pp = ctypes.cast(ctypes.pointer(p), ctypes.POINTER(_lib.PuctParams))
    one = ctypes.c_int64(0)
    ptr = ctypes.addressof(one)
    return L, {
        "search": lambda: L.gz_puct_search(ptr, ptr, 1, pp, ptr, ptr, ptr, ptr, ptr, None),
        "begin": lambda: L.gz_puct_begin(ptr, ptr, 1, pp, ptr, ptr, ptr, None),
        "run": lambda: L.gz_selfplay_puct_run(ptr, 1, pp, ptr, ptr, 1, ptr, 0, ptr, ptr, None),
        "run_active": lambda: L.gz_selfplay_puct_run_active(ptr, 1, 1, pp, ptr, ptr, 1, ptr, 0, ptr, ptr, None),
        "rounds": lambda: L.gz_selfplay_puct_rounds(ptr, 1, pp, ptr, ptr, 1, ptr, 0, ptr, ptr, None),
        "rounds_active": lambda: L.gz_selfplay_puct_rounds_active(ptr, 1, 1, pp, ptr, ptr, 1, ptr, 0, ptr, ptr, None)}


def _rejected(p, word):
    """Every entry point that takes the params returns GZ_ERR_ARG and names the cause (the
    checks come before every GPU call: any non-NULL pointer will do)."""
    L, calls = _calls(p)
    for name, call in calls.items():
        assert call() == -1 and word in L.gz_last_error(), (name, L.gz_last_error())


@pytest.mark.parametrize("kw", [dict(mc=0), dict(mc=33), dict(mc=-4), dict(cv=-1.0), dict(cv=1e4 + 1), dict(cv=float("nan")),
                                dict(cs=-0.5), dict(cs=1001.0), dict(cs=float("inf")), dict(gsc=-1.0), dict(gsc=8.01),
                                dict(gsc=float("nan"))])
def test_parameters_out_of_range_are_argument_errors(kw):
    _rejected(_raw(**kw), b"the Gumbel root needs")


@pytest.mark.parametrize("other", [_lib.GZ_PUCT_ROOT_NOISE, _lib.GZ_PUCT_LEAF_BATCH, _lib.GZ_PUCT_PLAYOUT_CAP,
                                   _lib.GZ_PUCT_FORCED_PLAYOUTS])
def test_the_flag_with_the_other_options_is_an_argument_error(other):
    _rejected(_raw(flags=_lib.GZ_PUCT_GUMBEL | other), b"the Gumbel root with")


def test_the_flag_with_tree_reuse_or_in_a_match_is_an_argument_error():
    for flags in (_lib.GZ_PUCT_GUMBEL, _lib.GZ_PUCT_GUMBEL | _lib.GZ_PUCT_LEAF_SYM):
        L, calls = _calls(_raw(flags=flags))
        for name in ("rounds", "rounds_active"):
            assert calls[name]() == -1 and b"the Gumbel root with tree reuse" in L.gz_last_error()
    p = _raw()
    one = ctypes.c_int64(0)
    ptr = ctypes.addressof(one)
    mp = _lib.PuctMatchParams(ctypes.cast(ctypes.pointer(p), ctypes.c_void_p), (ctypes.c_void_p * 2)(ptr, ptr),
                              (ctypes.c_int32 * 2)(_lib.GZ_PV_F16X3, _lib.GZ_PV_F16X3), 0, 0)
    assert L.gz_puct_match_run(ptr, 1, 1, ctypes.byref(mp), ptr, 1, ptr, 0, ptr, ptr, None) == -1
    assert b"the Gumbel root is not supported in a match" in L.gz_last_error()
    # without the flag nothing past the forced struct is read: a NaN there is not an error of its own
    q = _raw(cv=float("nan"), flags=0)
    pp = ctypes.cast(ctypes.pointer(q), ctypes.POINTER(_lib.PuctParams))
    assert L.gz_puct_search(None, None, 1, pp, None, None, None, None, None, None) == -1
    assert b"Gumbel" not in L.gz_last_error() and b"bad arguments" in L.gz_last_error()
    # with it, legal parameters pass the checks and fail on the buffers
    q = _raw()
    pp = ctypes.cast(ctypes.pointer(q), ctypes.POINTER(_lib.PuctParams))
    assert L.gz_puct_search(None, None, 1, pp, None, None, None, None, None, None) == -1
    assert b"Gumbel" not in L.gz_last_error() and b"bad arguments" in L.gz_last_error()


# ---------------------------------------------------------------- 7. the header alone, under the sanitizers
def _recurrence_rows():
    """The rows tests/hosttest/gumbel_main.cpp works on, by the same integer recurrence."""
    state = 20221004
    mask = (1 << 64) - 1

    def nxt():
        nonlocal state
        state = (state * 6364136223846793005 + 1442695040888963407) & mask
        return state >> 33

    nan = float("nan")
    rows = []
    for i in range(12):
        empty, prior, visits, W = [False] * CELLS, [0.0] * CELLS, [0] * CELLS, [0.0] * CELLS
        for c in range(CELLS):
            a, b, d, e = nxt(), nxt(), nxt(), nxt()
            empty[c] = a % 5 != 0
            prior[c] = float(1 + d % 1000) / 65536.0 if empty[c] else 0.0
            visits[c] = 1 + b % 7 if (empty[c] and b % 9 == 0) else 0
            W[c] = (float(e % 2001 - 1000) / 1000.0) * float(visits[c])
        if i == 1:
            for c in range(0, CELLS, 4):
                prior[c] = 0.0
            prior[1], prior[2] = float.fromhex("0x1p-1040"), nan
            empty[1] = empty[2] = True
        if i == 2:
            empty = [c in (7, 100, 224) for c in range(CELLS)]
        if i == 3:
            prior = [0.0 if c % 2 else nan for c in range(CELLS)]
        root = (7, 1000 + i, i, list(prior), list(empty), 16 if i % 2 else 1 + i, 0.0 if i == 4 else 1.0)
        if i == 1:
            visits = [9 if (c == 77 and empty[c]) else 0 for c in range(CELLS)]
        if i == 2:
            visits = [0] * CELLS
        for c in range(CELLS):
            if not empty[c]:
                prior[c], visits[c] = 0.0, 0
        pol = (prior, [True] * CELLS if i % 2 else empty, W, visits, float(i % 5 - 2) / 4.0)
        rows.append((root, pol))
    return rows


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_gumbel_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "gumbel_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", os.path.join(REPO, "tests", "hosttest", "gumbel_main.cpp"),
                    "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, \
        (r.stdout[-2000:], r.stderr[-2000:])
    lines = [x.split() for x in r.stdout.split("\n") if x.strip()]
    assert lines[-1] == ["ok"]
    seqs = [f for f in lines if f[0] == "seq"]
    assert len(seqs) == 30
    for f in seqs:
        assert [int(x) for x in f[3:]] == GR.seq(int(f[1]), int(f[2])), f[:3]
    rows = _recurrence_rows()
    by = {(f[0], int(f[1])): f for f in lines if f[0] in ("gs", "row", "pi")}
    assert len(by) == 3 * len(rows)
    for i, (root, pol) in enumerate(rows):
        gs, taken = GR.root(*root)
        f = by[("gs", i)]
        assert int(f[2]) == len(taken) and _bits([float.fromhex(x) for x in f[3:]]) == _bits(gs), i
        pi, row = GR.policy(*pol, 50.0, 0.5)
        assert [int(x) for x in by[("row", i)][2:]] == row, i
        assert _bits([float.fromhex(x) for x in by[("pi", i)][2:]]) == _bits(pi), i
    assert int(by[("gs", 2)][2]) == 3 and int(by[("gs", 3)][2]) == 16
