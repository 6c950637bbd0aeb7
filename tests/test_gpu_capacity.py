"""Full record and leaf buffers, and leaf tags across a device count.

The kernels that append to a caller's buffer reserve rows with an atomicAdd, write only
the rows below the capacity they were given and go on counting: selfplay_kernel and
selfplay_commit_kernel for the records of finished games (and the commit kernel for
their PUCT visit rows), LeafSink (csrc/gz_search.h) for the gathered leaves.  Here the
buffers are filled.

Method: every engine is built as usual, so each device buffer has its normal size; the
buffers a launch may write are filled with a sentinel byte; only the capacity handed to
the library (eng.record_cap / eng.leaf_cap, read at each launch) is lowered, never
raised.  The tail of the real buffer is then a guard band: a wrong bounds check writes
inside the allocation and fails the comparison with the sentinel.  Each case compares a
capped run with an uncapped run of an engine built with the same arguments: the rows
that fit are the uncapped run's rows bit for bit, the counters count what was lost, and
play goes on as if nothing had been dropped.

The order in which the slots of one launch reserve their records is not fixed, so
records are matched by (game_id, ply).  A single wavefront reserves its leaves in a
fixed order, so the leaf cases (one slot, one position) compare rows by index.

The planner path (gz_selfplay_plan_run) appends its records through the same
selfplay_commit_kernel as the PUCT paths, without visit rows, and its leaves through the
LeafSink of gz_plan_search, which has a case below: it needs no engine case of its own.

Every comparison is bitwise, except the tree forward's incremental rows, which use
test_gpu_pvinc's DELTA_TOL / 1e-6 (_close).
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import SEED
from gzero import _lib, boards, device, planner_nets, weights
from gzero.boards import RECORD_DTYPE, STATE_DTYPE
from gzero.device import ptr, stream
from gzero.selfplay import SelfPlayEngine
from test_gpu_pvinc import _close, _grand_family, _root_family, _rows

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
REC = RECORD_DTYPE.itemsize  # 80 bytes


def _fill(*tensors):
    for t in tensors:
        t.view(torch.uint8).fill_(SENTINEL)


def _bytes(t):
    return t.view(torch.uint8).cpu().numpy()


def _untouched(t, first_byte):
    return bool((_bytes(t)[first_byte:] == SENTINEL).all())


_PV = {}


def _pvw():
    if "w" not in _PV:
        _PV["w"] = device.PVWeights(weights.pack_pv_weights(weights.init_state_dict(0)), precision="f16x3")
    return _PV["w"]


# ---------------------------------------------------------------- A1 / A2: records (and visit rows)
def _fused_engine():
    # the engine of test_gpu_selfplay.test_selfplay_matches_reference_golden_games (beta 0):
    # games 100, 102 and 104 are 60, 71 and 75 plies long, so at least three games end in 100 plies
    return SelfPlayEngine(n_slots=6, num_simulations=2, c_puct=1.6, exploration=0.05, beta=0.0, seed=SEED,
                          plies_per_step=100, game_id_base=100, game_id_stride=6)


def _puct_engine(reuse):
    # a game ends by ply 200: every slot finishes a game within 200 plies, and within 600
    # rounds with tree reuse (a move takes at most num_simulations + 1 = 3 rounds)
    kw = dict(tree_reuse=True, rounds_per_step=600) if reuse else dict(plies_per_step=200)
    return SelfPlayEngine(n_slots=4, num_simulations=2, c_puct=1.6, seed=SEED, pv_weights=_pvw(), search="puct",
                          temp_plies=0, **kw)


ENGINES = {"fused": _fused_engine, "puct": lambda: _puct_engine(False), "puct_reuse": lambda: _puct_engine(True)}
_RUNS = {}


def _record_run(kind, cap=None):
    """One step of a fresh engine with record_cap lowered to `cap` (None: as allocated) ->
    counters, the whole record buffer (and visit buffer) as bytes, the boards afterwards."""
    eng = ENGINES[kind]()
    alloc = eng.record_cap
    assert eng.d_records.numel() == alloc * REC
    _fill(eng.d_records)
    if eng.d_visits is not None:
        assert eng.d_visits.numel() == alloc * 225
        _fill(eng.d_visits)
    if cap is not None:
        assert 0 <= cap <= alloc  # never above the allocation
        eng.record_cap = cap
    eng.step()
    torch.cuda.synchronize()
    st, gids = eng.boards()
    return {"counters": eng.counters().copy(), "alloc": alloc, "records": _bytes(eng.d_records),
            "visits": None if eng.d_visits is None else _bytes(eng.d_visits), "boards": st.tobytes(),
            "gids": [int(g) for g in gids]}


def _uncapped(kind):
    """The uncapped run of an engine kind: made once, shared by its cases, left unchanged."""
    if kind not in _RUNS:
        run = _record_run(kind)
        c = run["counters"]
        T = int(c["records"])
        assert c["records_dropped"] == 0 and c["games"] >= (3 if kind == "fused" else 4) and 0 < T <= run["alloc"]
        assert (run["records"][T * REC:] == SENTINEL).all()
        recs = np.frombuffer(run["records"][:T * REC].tobytes(), RECORD_DTYPE)
        keys = [(int(g), int(p)) for g, p in zip(recs["game_id"], recs["ply"])]
        assert len(set(keys)) == T
        run["rows"] = {k: run["records"][i * REC:(i + 1) * REC].tobytes() for i, k in enumerate(keys)}
        if run["visits"] is not None:
            assert (run["visits"][T * 450:] == SENTINEL).all()
            run["vrows"] = {k: run["visits"][i * 450:(i + 1) * 450].tobytes() for i, k in enumerate(keys)}
            vis = run["visits"][:T * 450].view(np.uint16).reshape(T, 225)
            assert (vis.sum(axis=1) == 2).all()  # real visit rows: num_simulations visits each
        run["T"] = T
        _RUNS[kind] = run
    return _RUNS[kind]


CAPS = ["0", "1", "T//2", "T-1", "T"]


def _cap_of(name, T):
    return {"0": 0, "1": 1, "T//2": T // 2, "T-1": T - 1, "T": T}[name]


def _check_records(kind, cap_name):
    full = _uncapped(kind)
    T = full["T"]
    cap = _cap_of(cap_name, T)
    got = _record_run(kind, cap)
    c, fc = got["counters"], full["counters"]
    print(kind, "T", T, "cap", cap, "counters", c)
    assert int(c["records"]) == T
    assert int(c["records_dropped"]) == max(0, T - cap)
    for k in ("moves", "games", "mcts_moves"):
        assert c[k] == fc[k], k
    n = min(cap, T)
    recs = np.frombuffer(got["records"][:n * REC].tobytes(), RECORD_DTYPE)
    keys = [(int(g), int(p)) for g, p in zip(recs["game_id"], recs["ply"])]
    assert len(set(keys)) == n  # no (game_id, ply) twice
    for i, k in enumerate(keys):
        assert k in full["rows"], k
        assert got["records"][i * REC:(i + 1) * REC].tobytes() == full["rows"][k], (i, k)
        if full["visits"] is not None:
            assert got["visits"][i * 450:(i + 1) * 450].tobytes() == full["vrows"][k], (i, k)
    # a game's surviving rows: consecutive, in ply order, from ply 0
    for g in np.unique(recs["game_id"]):
        idx = np.flatnonzero(recs["game_id"] == g)
        assert np.array_equal(idx, np.arange(idx[0], idx[0] + len(idx))), int(g)
        assert np.array_equal(recs["ply"][idx], np.arange(len(idx))), int(g)
    # the guard band: every byte past the capacity is still the sentinel
    assert (got["records"][cap * REC:] == SENTINEL).all()
    if full["visits"] is not None:
        assert (got["visits"][cap * 450:] == SENTINEL).all()
    # dropping records does not change play
    assert got["boards"] == full["boards"] and got["gids"] == full["gids"]
    if cap_name == "1" and kind == "fused":
        # three or more finished games: one straddles the end, the others lie wholly past it
        assert int(fc["games"]) >= 3 and T >= 206


@pytest.mark.parametrize("cap", CAPS)
def test_full_record_buffer_fused_kernel(cap):
    """selfplay_kernel (gz_selfplay_run): 6 slots x 100 plies in one launch."""
    _check_records("fused", cap)


@pytest.mark.parametrize("reuse", [False, True], ids=["lockstep", "tree_reuse"])
@pytest.mark.parametrize("cap", CAPS)
def test_full_record_buffer_commit_kernel(cap, reuse):
    """selfplay_commit_kernel with the PUCT visit rows (gz_selfplay_puct_run, and
    gz_selfplay_puct_rounds with tree reuse): row i of d_visits belongs to record i."""
    _check_records("puct_reuse" if reuse else "puct", cap)


# ---------------------------------------------------------------- A3: leaves
def _leaf_run(cap=None):
    """One slot, one ply, with the tree forward of the gathered leaves."""
    eng = SelfPlayEngine(n_slots=1, num_simulations=16, beta=0.0, seed=SEED, pv_weights=_pvw(), pv_mode="tree",
                         plies_per_step=1)
    eng.advance(10)
    before, _ = eng.boards()
    alloc = eng.leaf_cap
    bufs = {"leaves": eng.d_leaves, "meta": eng.d_meta, "logits": eng.d_logits, "value": eng.d_value,
            "probs": eng.d_probs, "prior": eng.d_prior}
    _fill(*bufs.values())
    eng.d_tree_ws.zero_()  # (with capacity 0 nothing runs: the list sizes read are these zeros)
    if cap is not None:
        assert 0 <= cap <= alloc
        eng.leaf_cap = cap
    eng.step()
    torch.cuda.synchronize()
    after, gids = eng.boards()
    out = {k: _bytes(t) for k, t in bufs.items()}
    out.update(counters=eng.counters().copy(), alloc=alloc, stats=eng.tree_stats(), before=before.copy(),
               after=after.copy(), gids=[int(g) for g in gids])
    return out


def _uncapped_leaves():
    if "leaves" not in _RUNS:
        run = _leaf_run()
        n = int(run["counters"]["leaves"])
        assert 2 <= n <= run["alloc"]
        _RUNS["leaves"] = run
    return _RUNS["leaves"]


def _move_played(run):
    b, a = run["before"][0], run["after"][0]
    d = boards.words_to_cells(a["black"], a["white"]).astype(int) - boards.words_to_cells(b["black"], b["white"])
    return [(int(cell), int(d[cell])) for cell in np.flatnonzero(d)]


@pytest.mark.parametrize("cap_name", ["0", "1", "n//2", "n-1"])
def test_full_leaf_buffer_engine(cap_name):
    """LeafSink through gz_selfplay_run, then gz_pv_forward_tree with the count above
    its n (what a full leaf buffer hands it): 16 simulations after 10 plies."""
    full = _uncapped_leaves()
    n_a = int(full["counters"]["leaves"])
    cap = {"0": 0, "1": 1, "n//2": n_a // 2, "n-1": n_a - 1}[cap_name]
    got = _leaf_run(cap)
    print("leaves", n_a, "cap", cap, "tree stats", got["stats"])
    assert int(got["counters"]["leaves"]) == n_a  # the counter keeps counting past the capacity
    assert got["counters"]["moves"] == 1
    assert np.array_equal(got["leaves"][:cap * 64], full["leaves"][:cap * 64])
    assert np.array_equal(got["meta"][:cap * 4], full["meta"][:cap * 4])
    for k, width in (("leaves", 64), ("meta", 4), ("logits", 900), ("value", 4), ("probs", 900), ("prior", 1800)):
        assert (got[k][cap * width:] == SENTINEL).all(), k
    st = got["stats"]
    assert st[1] + st[2] + st[3] + st[4] == cap, st
    if cap:
        rows = got["leaves"][:cap * 64].view(np.uint32).reshape(cap, 16)
        meta = got["meta"][:cap * 4].view(np.int32)
        ref = device.pv_forward(_pvw(), rows, want_prior=True)
        tree = (got["logits"][:cap * 900].view(np.float32), got["value"][:cap * 4].view(np.float32),
                got["probs"][:cap * 900].view(np.float32), got["prior"][:cap * 1800].view(np.float64))
        assert meta[0] == -1
        _close(ref, tree, cap, np.flatnonzero(meta == -1))
    assert _move_played(got) == _move_played(full)
    assert got["after"].tobytes() == full["after"].tobytes() and got["gids"] == full["gids"]


def _position():
    """A 10-stone position (black to move)."""
    cells = np.zeros(225, np.int8)
    for k, m in enumerate([112, 113, 97, 128, 111, 127, 96, 98, 126, 142]):
        cells[m] = 1 + k % 2
    return boards.make_states(cells[None], n_moves=10, player=1)


def _raw_search(params, leaf_cap, alloc_rows, plan=None):
    """gz_search / gz_plan_search (plan = (planner params, GNWeights)) of _position() with a
    sentinel-filled leaf buffer of alloc_rows >= leaf_cap rows -> (move, stats bytes,
    *d_leaf_count, the whole leaf buffer as bytes)."""
    lib = device.require_gpu()
    assert 0 <= leaf_cap <= alloc_rows
    d_states = device.to_dev(_position())
    d_gids = torch.tensor([3], dtype=torch.int64, device="cuda")
    d_moves = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_stats = torch.zeros(ctypes.sizeof(_lib.SearchStats), dtype=torch.uint8, device="cuda")
    d_leaves = torch.empty(alloc_rows * 16, dtype=torch.int32, device="cuda")
    _fill(d_leaves)
    d_lc = torch.zeros(1, dtype=torch.int32, device="cuda")
    if plan is None:
        _lib.check(lib.gz_search(ptr(d_states), ptr(d_gids), 1, ctypes.byref(params), None, ptr(d_moves),
                                 ptr(d_stats), ptr(d_leaves), int(leaf_cap), ptr(d_lc), stream()), "gz_search")
    else:
        pparams, gnw = plan
        ws = torch.empty(lib.gz_plan_workspace_bytes(1, params.num_simulations), dtype=torch.uint8, device="cuda")
        _lib.check(lib.gz_plan_search(ptr(d_states), ptr(d_gids), 1, ctypes.byref(params), ctypes.byref(pparams),
                                      ptr(gnw.tensor), ptr(ws), None, ptr(d_moves), ptr(d_stats), ptr(d_leaves),
                                      int(leaf_cap), ptr(d_lc), stream()), "gz_plan_search")
    torch.cuda.synchronize()
    return int(d_moves.item()), _bytes(d_stats).tobytes(), int(d_lc.item()), _bytes(d_leaves)


def _check_search_caps(params, caps, plan=None):
    alloc = params.num_simulations + 1
    mv, stats, n, rows = _raw_search(params, alloc, alloc, plan)
    assert 2 <= n <= alloc and mv >= 0
    assert (rows[n * 64:] == SENTINEL).all() and not (rows[:n * 64].view(np.uint32) == 0xA5A5A5A5).any()
    for cap in caps(n):
        assert 0 <= cap < n
        mv2, stats2, n2, rows2 = _raw_search(params, cap, alloc, plan)
        assert n2 == n, (cap, n2, n)  # the count goes on past the capacity
        assert np.array_equal(rows2[:cap * 64], rows[:cap * 64]), cap
        assert (rows2[cap * 64:] == SENTINEL).all(), cap  # the guard rows
        assert mv2 == mv and stats2 == stats, cap
    return n


def test_full_leaf_buffer_gz_search():
    """gz_search with leaf_cap below the leaves it produces.  16 simulations: the root
    and its children, reserved at once.  250 simulations: past the 215 children the
    search reserves a leaf at a time, and a capacity of 220 ends between those."""
    p = device.search_params(16, 1.6, 0.05, 0.0, SEED, gather_leaves=True)
    _check_search_caps(p, lambda n: (0, 1, n // 2, n - 1))
    p = device.search_params(250, 1.6, 0.05, 0.0, SEED, gather_leaves=True)
    n = _check_search_caps(p, lambda n: (100, 220, n - 1))
    assert n > 221


def test_full_leaf_buffer_gz_plan_search():
    """gz_plan_search (8 simulations, planner_steps 1) with leaf_cap below its leaves."""
    gnw = device.GNWeights(planner_nets.pack_planner_weights(planner_nets.init_graphnet_state(0),
                                                             planner_nets.init_dqn_state(1)))
    p = device.search_params(8, 1.6, 0.05, 0.2, SEED, planner_steps=1, gather_leaves=True)
    _check_search_caps(p, lambda n: (0, 1, n // 2, n - 1), plan=(_lib.planner_params("medium"), gnw))


# ---------------------------------------------------------------- A4: tags across a count
def test_tree_tags_across_a_device_count():
    """gz_pv_forward_tree with a d_count inside the list: the count cuts between the
    children of root C; a child of root B stands before B; a child of root D, which lies
    past the count, stands before it.  Rows below the count are within DELTA_TOL of the
    full forward; the roots and the row whose tagged parent is past the count take the
    full kernel (bitwise); nothing past the count is written."""
    rng = np.random.default_rng(SEED + 40)
    pvw = _pvw()
    root_b, kids_b = _root_family(rng, 24)
    root_c, kids_c = _root_family(rng, 61)
    root_d, kids_d = _root_family(rng, 12)
    fam_a, meta_a = _grand_family(rng, 33, [0, 112, 119], every=9)
    cells, meta = [kids_b[5], kids_d[7]], [None, None]
    cells += fam_a
    meta += [m + 2 if m >= 0 else m for m in meta_a]
    ib = len(cells)
    cells.append(root_b)
    meta.append(-1)
    cells += kids_b[10:30]
    meta += [ib] * 20
    ic = len(cells)
    cells.append(root_c)
    meta.append(-1)
    cells += kids_c[:20]
    meta += [ic] * 20
    count = ic + 1 + 10  # between root C's children
    i_d = len(cells)
    cells.append(root_d)
    meta.append(-1)
    cells += kids_d[20:30]
    meta += [i_d] * 10
    meta[0], meta[1] = ib, i_d
    n = len(cells)
    assert ib < count <= i_d < n
    rows = _rows(cells)
    full = device.pv_forward(pvw, rows, want_prior=True)
    tree = device.pv_forward_tree(pvw, rows, meta, d_count=count)
    st = tree[4]
    n_gc = sum(1 for m in meta_a if m > 0)
    # roots A, B, C; children: A's, B's 20 and the one before B, C's first 10; the row tagged
    # with root D is the one full-forward board
    assert st[:5] == [3, 3, (len(fam_a) - 1 - n_gc) + 21 + 10, 1, n_gc], (st, n_gc)
    below = [np.asarray(x).reshape(n, -1)[:count] for x in tree[:4]]
    ref = [np.asarray(x).reshape(n, -1)[:count] for x in full[:4]]
    exact = [2, ib, ic, 1]
    print("tags across a count:", _close(ref, below, count, exact))
    nan32 = torch.full((1,), float("nan"), dtype=torch.float32).numpy().view(np.uint32)[0]
    nan64 = torch.full((1,), float("nan"), dtype=torch.float64).numpy().view(np.uint64)[0]
    for x, bits, pat in zip(tree[:4], (np.uint32, np.uint32, np.uint32, np.uint64), (nan32, nan32, nan32, nan64)):
        past = np.ascontiguousarray(np.asarray(x).reshape(n, -1)[count:])
        assert (past.view(bits) == pat).all()
