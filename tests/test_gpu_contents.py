"""No entry point may depend on what its buffers held before the call.

Every case runs one call (or one engine) through the existing wrappers four times, the
``torch.empty`` of the wrappers replaced by tests/devmem.py:

1. every workspace and every output the header promises to write filled with 0x00;
2. 0x00 again -- the determinism baseline;
3. filled with 0xFF (ints of -1; fp16 / fp32 / fp64 NaN);
4. "leftover": a larger valid call of the same entry point (an earlier whole run where
   the table of the issue names none) under 0xFF first, then the case on the SAME
   buffers, not filled at all.

Every documented output of runs 2, 3 and 4 must equal run 1's bit for bit
(``tobytes()``), and after every run the 64 KB guard band behind every allocation must
still hold 0xA5: a kernel that reads workspace it never wrote, leaves a promised output
unwritten or writes past a ``gz_*_workspace_bytes`` fails here.  No tolerance is involved.

Documented fields only, where the header says so: a search tree is compared at entries
[0, n_nodes) of every array; output rows at or past ``*d_count`` / ``leaf_cap`` / the
record count are not written and must still hold the fill.

One finding is built into the comparisons (runs 1 and 2 already differ in it): the ROW
ORDER of gathered leaves (and of everything computed per leaf row) and of the records of
games that end in the same launch is set by integer atomics (leaf_reserve, the record
counter), so it varies from run to run.  Those tables are compared as multisets of whole
rows -- (leaf, tag class, logits, value, probs, prior) or (record, visit row) sorted by
their bytes -- still bit for bit; no floating-point output differs between runs.  When
the leaf buffer overflows, which leaves are dropped depends on that order too: the kept
rows are then required to be rows of the uncapped call.

Who initialises what a kernel reads before writing it (from the host functions):

    entry point                 region                               initialised by
    gz_pv_forward               head records' K-padding floats       the tower kernels (zeros)
    gz_pv_forward_tree          counters, queue heads; ghead         hipMemsetAsync (0; 0xFF)
                                ord, pslot, cinfo, wcount            tree_roots / tree_lists kernels
                                gnext, roots / full / grand lists    written up to their counts only
    gz_gn_forward_chain         list counts, queue head              hipMemsetAsync
    gz_plan_search              both counter sets, the jobs          hipMemsetAsync
                                GraphNet statistics                  the caller's first reset (header)
    gz_puct_begin / _search     config, tree header, node 0, pend    puct_begin_kernel
                                a node's prior row                   its backup; zeros if never evaluated
                                the batched search's `left`          hipMemsetAsync
    gz_selfplay_puct_rounds     reuse marks of the trees             gz_selfplay_puct_reset (header)
    gz_selfplay_init            every slot's 128-byte header         selfplay_init_kernel
    gz_sgd_forward / _backward  weight scales                        hipMemsetAsync
                                xmax / dymax, BN and weight partials the conv kernels, every board
    gz_adam_step                norm partials                        adam_norm_kernel, every block

The only place where the poison is meant to be visible is
``test_tree_stats_show_the_poison``.  Nothing here calls an API against its contract.
"""
import copy
import ctypes
import random

import numpy as np
import pytest
import torch
import torch.nn as nn

import devmem
from conftest import SEED, golden
from gzero import _lib, boards, device, planner_nets, rng, weights
from gzero.boards import RECORD_DTYPE, STATE_DTYPE

pytestmark = pytest.mark.gpu

FILLS = ("0x00", "0x00 again", "0xFF", "leftover")


# ---------------------------------------------------------------- the four runs
def _b(x):
    """The bytes of an output."""
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    if isinstance(x, (bytes, bytearray)):
        return bytes(x)
    return np.ascontiguousarray(x).tobytes()


def _rows_sorted(*cols):
    """Tables with one row per item (same row count), joined and sorted by the rows' bytes:
    the multiset of the joined rows."""
    n = len(cols[0])
    parts = []
    for c in cols:
        if isinstance(c, torch.Tensor):
            c = c.detach().cpu().numpy()
        c = np.ascontiguousarray(c)
        assert len(c) == n
        parts.append(c.view(np.uint8).reshape(n, -1) if n else np.zeros((0, 1), np.uint8))
    a = np.ascontiguousarray(np.concatenate(parts, axis=1))
    if n == 0:
        return a
    return a[np.argsort(a.view(np.dtype((np.void, a.shape[1]))).ravel(), kind="stable")]


def _tree_bytes(trees):
    """Parsed trees (dicts of arrays already cut to n_nodes) -> one bytes value."""
    out = []
    for t in trees:
        for k in sorted(t):
            out.append(k.encode() + b"=" + _b(np.asarray(t[k])))
    return b"|".join(out)


def _holds(t, pattern):
    """Every byte of a tensor slice still holds the fill."""
    raw = t.detach().contiguous().view(torch.uint8) if t.numel() else t
    return bool((raw == pattern).all())


def _four_fills(case, larger=None):
    """case(mem, state) -> {name: bytes}; larger(mem) -> state (an object whose buffers the
    leftover run uses again, or None when the wrappers allocate per call: those allocations
    then take the larger call's buffers by call site, devmem's ``reuse``)."""
    outs = []
    for pat in (0x00, 0x00, 0xFF):
        with devmem.poisoned(pat) as mem:
            outs.append(case(mem, None))
            torch.cuda.synchronize()
            mem.check()
    with devmem.poisoned(0xFF) as big:
        state = larger(big) if larger is not None else (case(big, None), None)[1]
        torch.cuda.synchronize()
        big.check()
    with devmem.poisoned(devmem.LEFTOVER, reuse=big) as mem:
        outs.append(case(mem, state))
        torch.cuda.synchronize()
        mem.check()
        assert state is not None or mem.reused() or not mem.allocations, "the leftover run got fresh buffers"
    big.check()  # (a kept object's workspace is the larger call's allocation)
    for k in range(1, 4):
        assert outs[k].keys() == outs[0].keys()
        diff = [name for name in outs[0] if outs[k][name] != outs[0][name]]
        assert not diff, f"fill {FILLS[k]}: {diff} differ from the {FILLS[0]} run"
    assert all(len(v) > 0 for v in outs[0].values()), [k for k, v in outs[0].items() if not v]
    return outs[0]


# ---------------------------------------------------------------- inputs (made once, never changed)
_CACHE = {}


def _once(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _pv_blob(seed=0):
    return _once(("pv", seed), lambda: weights.pack_pv_weights(weights.init_state_dict(seed)))


def _gn_blob():
    return _once("gn", lambda: planner_nets.pack_planner_weights(planner_nets.init_graphnet_state(0),
                                                                planner_nets.init_dqn_state(1)))


def _random_rows(n, seed):
    def make():
        r = np.random.default_rng(seed)
        cells = r.choice(3, size=(n, 225), p=[0.5, 0.25, 0.25]).astype(np.int8)
        cells[0] = 0
        bl, wh = boards.cells_to_words(cells)
        return boards.leaf_words(bl, wh)
    return _once(("rows", n, seed), make)


def _pattern_cells():
    """A full board with no run longer than two in any direction."""
    return np.array([1 + ((c // 2 + r) % 2) for r in range(15) for c in range(15)], np.int8)


def _thinned(keep, seed):
    cells = _pattern_cells()
    cells[np.random.RandomState(seed).permutation(225)[keep:]] = 0
    return cells


def _positions(n, seed, finished=True):
    """n search roots without a five: the empty board, sparse and dense boards, one with
    three empty cells (terminal nodes in every tree) and, with ``finished``, one that is
    over."""
    keeps = [0, 40, 121, 222, 100, 8, 64, 200, 150, 30, 90, 219]
    st = np.concatenate([boards.make_states(_thinned(keeps[i % len(keeps)], seed + i)[None]) for i in range(n)])
    if finished and n > 4:
        st["over"][4] = 1
    return st


# ---------------------------------------------------------------- gz_pv_forward
@pytest.mark.parametrize("precision", ["fp32", "f16x3", "f16"])
def test_pv_forward(precision):
    rows, big_rows = _random_rows(130, 1), _random_rows(700, 2)

    def larger(mem):
        w = device.PVWeights(_pv_blob(), precision)
        device.pv_forward(w, big_rows, want_prior=True)
        return w

    def case(mem, w):
        w = w or device.PVWeights(_pv_blob(), precision)
        lg, v, pr, prior = device.pv_forward(w, rows, want_prior=True)
        return {"logits": _b(lg), "value": _b(v), "probs": _b(pr), "prior": _b(prior)}

    out = _four_fills(case, larger)
    assert np.isfinite(np.frombuffer(out["logits"], np.float32)).all()


@pytest.mark.parametrize("precision", ["fp32", "f16x3", "f16"])
def test_pv_forward_device_count(precision):
    """Capacity 130, 70 boards: rows >= 70 of every output keep the fill."""
    cap, cnt = 130, 70
    rows = _random_rows(cap, 1)

    def case(mem, _):
        w = device.PVWeights(_pv_blob(), precision)
        d_b = torch.from_numpy(rows.view(np.int32).copy()).cuda()
        d_count = torch.tensor([cnt], dtype=torch.int32, device="cuda")
        d_probs = mem.torch.empty(cap * 225, dtype=torch.float32, device="cuda")
        d_prior = mem.torch.empty(cap * 225, dtype=torch.float64, device="cuda")
        lg, v, _ = device.pv_forward_dev(w, d_b, cap, d_count=d_count, d_probs=d_probs, d_prior=d_prior)
        torch.cuda.synchronize()
        if mem.pattern != devmem.LEFTOVER:
            for t, width in ((lg, 225), (v, 1), (d_probs, 225), (d_prior, 225)):
                assert _holds(t[cnt * width:], mem.pattern), "a row at or past *d_count was written"
        return {"logits": _b(lg[: cnt * 225]), "value": _b(v[:cnt]), "probs": _b(d_probs[: cnt * 225]),
                "prior": _b(d_prior[: cnt * 225])}

    _four_fills(case)


# ---------------------------------------------------------------- gz_pv_forward_tree
def _tree_family(rng_, ns, grand, untagged):
    """A root of ns stones, a child on every empty cell, `grand` grandchildren (under the
    first children, tagged with their parent) and `untagged` deeper nodes (-2)."""
    from test_gpu_pvinc import _root_family
    root, kids = _root_family(rng_, ns)
    mover = 1 if ns % 2 == 0 else 2
    cells, meta = [root] + kids, [-1] + [0] * len(kids)
    for k in range(grand):
        g = kids[k].copy()
        g[np.flatnonzero(g == 0)[3 * k]] = 3 - mover
        cells.append(g)
        meta.append(1 + k)
    for k in range(untagged):
        g = kids[-1 - k].copy()
        e = np.flatnonzero(g == 0)
        g[e[0]], g[e[1]] = 3 - mover, mover
        cells.append(g)
        meta.append(-2)
    return cells, meta


def _tree_inputs():
    def make():
        from test_gpu_pvinc import _concat, _rows
        r = np.random.default_rng(SEED)
        fams = [_tree_family(r, ns, 5, 3) for ns in (4, 40, 150)]
        cells, meta = _concat(fams)
        c1, m1 = fams[0]
        return (_rows(cells), np.asarray(meta, np.int32)), (_rows(c1), np.asarray(m1, np.int32))
    return _once("tree", make)


def _tree_call(mem, rows, meta, root_cap):
    lib = _lib.load()
    w = device.PVWeights(_pv_blob(), "f16x3")
    lg, v, pr, prior, stats = device.pv_forward_tree(w, rows, meta, root_cap=root_cap)
    ws = max(mem.allocations, key=lambda a: a.nbytes)
    assert ws.nbytes == lib.gz_pv_tree_workspace_bytes(len(rows), root_cap)
    tiles = mem.torch.empty(2, dtype=torch.int32, device="cuda")
    _lib.check(lib.gz_pv_tree_exec_tiles(device.ptr(ws.base), len(rows), device.ptr(tiles), device.stream()),
               "gz_pv_tree_exec_tiles")
    return {"logits": _b(lg), "value": _b(v), "probs": _b(pr), "prior": _b(prior),
            "tree_stats": _b(np.asarray(stats, np.int32)), "exec_tiles": _b(tiles)}, stats


def test_pv_forward_tree():
    """One root with a child on every empty cell, 5 grandchildren and 3 untagged nodes,
    root_cap 1; the leftover run follows the three-family call (root_cap 3) on the same
    workspace, whose regions then lie elsewhere."""
    (rows3, meta3), (rows1, meta1) = _tree_inputs()

    def larger(mem):
        out, stats = _tree_call(mem, rows3, meta3, 3)
        assert stats[:2] == [3, 3] and stats[4] == 15
        return None

    def case(mem, _):
        out, stats = _tree_call(mem, rows1, meta1, 1)
        kids = int((meta1 == 0).sum())
        assert stats == [1, 1, kids, 3, 5, 5], stats
        return out

    _four_fills(case, larger)


def test_tree_stats_show_the_poison():
    """The poison reaches the library and can be seen: gz_pv_tree_stats copies six counters
    out of the workspace and dereferences nothing.  On a workspace no forward has used it
    returns the fill; after one gz_pv_forward_tree the true counts under both fills."""
    lib = _lib.load()
    (_, _), (rows1, meta1) = _tree_inputs()
    n = len(rows1)
    for pat, want in ((0xFF, [-1] * 6), (0x00, [0] * 6)):
        with devmem.poisoned(pat) as mem:
            ws = mem.torch.empty(lib.gz_pv_tree_workspace_bytes(n, 1), dtype=torch.uint8, device="cuda")
            st = torch.zeros(6, dtype=torch.int32, device="cuda")
            _lib.check(lib.gz_pv_tree_stats(device.ptr(ws), n, device.ptr(st), device.stream()), "gz_pv_tree_stats")
            assert st.cpu().tolist() == want
            out, stats = _tree_call(mem, rows1, meta1, 1)
            assert stats == [1, 1, int((meta1 == 0).sum()), 3, 5, 5], (pat, stats)


# ---------------------------------------------------------------- gz_gn_forward(_chain)
@pytest.mark.parametrize("logits", [False, True])
def test_gn_forward(logits):
    """n = 33: without logits the heads run split over output tiles (the layers' outputs go
    through the workspace), with logits batched."""
    rows, big_rows = _random_rows(33, 3), _random_rows(300, 4)

    def run(w, r):
        if logits:
            return device.gn_forward(w, r)
        d_b = torch.from_numpy(r.view(np.int32).copy()).cuda()
        p, q, _ = device.gn_forward_dev(w, d_b, len(r))
        torch.cuda.synchronize()
        return p, q

    def larger(mem):
        w = device.GNWeights(_gn_blob())
        run(w, big_rows)
        return w

    def case(mem, w):
        out = run(w or device.GNWeights(_gn_blob()), rows)
        return {name: _b(x) for name, x in zip(("p", "q", "logits"), out)}

    _four_fills(case, larger)


GN_TAG = np.dtype([("mode", "<i4"), ("base", "<i4"), ("job", "<i4"), ("cell", "<i4"), ("nst", "<i4"),
                   ("st", "u1", (6,)), ("pad", "u1", (2,)), ("pad2", "<i4")])


def _gn_chains(mem, w, R, seed):
    """R bases (full forward, maps kept in slots 0..R-1), then 3 plies adding a stone each
    into job slots R..2R-1 (a full forward inside some chains): p and q of every call.
    Slots, workspace and outputs all come from the shim."""
    lib = _lib.load()
    r = np.random.default_rng(seed)
    d_slots = mem.torch.empty(2 * R * lib.gz_gn_slot_bytes(), dtype=torch.uint8, device="cuda")
    out = {}

    def forward(cells, tags, name):
        bl, wh = boards.cells_to_words(np.asarray(cells, np.int8))
        d_b = torch.from_numpy(boards.leaf_words(bl, wh).view(np.int32).copy()).cuda()
        d_t = torch.from_numpy(np.ascontiguousarray(tags).view(np.uint8).copy()).cuda()
        d_p = mem.torch.empty(R * 225, dtype=torch.float32, device="cuda")
        d_q = mem.torch.empty(R * 225, dtype=torch.float32, device="cuda")
        ws = mem.torch.empty(lib.gz_gn_chain_workspace_bytes(R), dtype=torch.uint8, device="cuda")
        _lib.check(lib.gz_gn_forward_chain(device.ptr(w.tensor), device.ptr(d_b), R, device.ptr(d_t),
                                           device.ptr(d_slots), device.ptr(d_p), device.ptr(d_q), device.ptr(ws),
                                           device.stream()), "gz_gn_forward_chain")
        torch.cuda.synchronize()
        out[name + ".p"], out[name + ".q"] = _b(d_p), _b(d_q)

    cur = r.choice(3, size=(R, 225), p=[0.7, 0.15, 0.15]).astype(np.int8)
    cur[0] = 0
    tags = np.zeros(R, GN_TAG)
    tags["job"] = np.arange(R)
    forward(cur, tags, "base")
    stones, rebased = [[] for _ in range(R)], np.zeros(R, bool)
    corners = [0, 14, 210, 224, 7, 105, 119, 217]
    for ply in range(3):
        tags = np.zeros(R, GN_TAG)
        for g in range(R):
            pref = [c for c in corners if cur[g][c] == 0]
            c = int(pref[(g + ply) % len(pref)]) if (g % 3 == 0 and pref) else int(r.choice(np.flatnonzero(cur[g] == 0)))
            cur[g][c] = 1 + (ply + g) % 2
            t = tags[g]
            t["job"] = R + g
            if g % 5 == 4 and ply == 1:  # a full forward inside the chain
                t["mode"], t["base"] = 0, R + g
                rebased[g], stones[g] = True, []
            else:
                t["mode"], t["cell"] = 1, c
                t["base"] = R + g if rebased[g] else g
                t["nst"] = 0 if rebased[g] else len(stones[g])
                for k, s in enumerate(stones[g]):
                    t["st"][k] = s
                if not rebased[g]:
                    stones[g].append(c)
        forward(cur, tags, f"ply{ply}")
    return out


def test_gn_forward_chain():
    def larger(mem):
        _gn_chains(mem, device.GNWeights(_gn_blob()), 23, 12)  # more rows, more slots
        return None

    _four_fills(lambda mem, _: _gn_chains(mem, device.GNWeights(_gn_blob()), 10, 11), larger)


# ---------------------------------------------------------------- planner move, knowledge scores
def test_planner_move_and_knowledge_scores():
    small, big = _positions(5, 50, finished=False), _positions(70, 51, finished=False)
    pp = _lib.planner_params("medium")

    def run(st):
        n = len(st)
        gnw = device.GNWeights(_gn_blob())
        keys = [rng.stream_key(SEED, i, int(st["n_moves"][i]), 1) for i in range(n)]
        ais = [1 + i % 2 for i in range(n)]
        mv, dr = device.planner_move(st, ais, keys, pp, gnw)
        sc = device.knowledge_scores(st, [int(p) for p in st["player"]])
        return {"moves": _b(mv), "draws": _b(dr), "scores": _b(sc)}

    _four_fills(lambda mem, _: run(small), lambda mem: (run(big), None)[1])


# ---------------------------------------------------------------- K1, rollout policy, rollouts, patterns
def test_board_step_policy_rollout_pattern(oracle):
    """No workspace: the point is the outputs, which the wrappers now allocate with
    torch.empty -- ok = 0 of an illegal move (-1 / 225 / 1000, a finished board) has to be
    stored by the kernel."""
    from test_gpu_kernels import _states_from_moves
    pol = golden("policy")["cases"][:70]
    rol = golden("rollout")["cases"][:70]
    pat = golden("pattern")["positions"][:70]
    st_pol = _states_from_moves(oracle, [c["moves"] for c in pol])
    st_rol = _states_from_moves(oracle, [c["moves"] for c in rol])
    st_pat = _states_from_moves(oracle, [c["moves"] for c in pat])
    crafted = boards.make_states(np.zeros((6, 225), np.int8))
    crafted["over"][5] = 1
    keys_pol = [rng.stream_key(SEED, i, len(c["moves"]), 1) for i, c in enumerate(pol)]
    keys_rol = [rng.stream_key(SEED, i, len(c["moves"]), 1) for i, c in enumerate(rol)]

    def case(mem, _):
        out = {}
        new, ok, legal = device.board_step(crafted, [-1, 225, 1000, 3, 224, 7])
        assert list(ok) == [0, 0, 0, 1, 1, 0]
        out["step.states"], out["step.ok"], out["step.legal"] = _b(new), _b(ok), _b(legal)
        new, ok, legal = device.board_step(st_pol, [c["move"] for c in pol])
        out["step2.states"], out["step2.ok"], out["step2.legal"] = _b(new), _b(ok), _b(legal)
        mv, dr = device.policy_move(st_pol, keys_pol)
        assert list(mv) == [c["move"] for c in pol] and list(dr) == [c["draws"] for c in pol]
        out["policy.moves"], out["policy.draws"] = _b(mv), _b(dr)
        vals, fin, dr = device.rollout(st_rol, [c["player"] for c in rol], keys_rol)
        assert list(vals) == [c["value"] for c in rol]
        out["rollout.values"], out["rollout.final"], out["rollout.draws"] = _b(vals), _b(fin), _b(dr)
        for pl in (1, 2):
            s, bg = device.pattern_score(st_pat, [pl] * len(pat))
            assert list(s) == [c[f"s{pl}"] for c in pat]
            out[f"pattern{pl}.score"], out[f"pattern{pl}.bg"] = _b(s), _b(bg)
        return out

    _four_fills(case)


# ---------------------------------------------------------------- gz_search, gz_plan_search
def _search_out(mv, stats, trees, leaves, all_leaves, cap):
    out = {"moves": _b(mv), "stats": _b(stats), "trees": _tree_bytes(trees)}
    if all_leaves is None:
        out["leaves"] = _b(_rows_sorted(leaves))
    else:  # the buffer overflowed: which rows were dropped depends on the atomics' order
        assert len(leaves) == cap
        have = {bytes(r) for r in all_leaves.view(np.uint8).reshape(len(all_leaves), -1)}
        assert all(bytes(r) in have for r in leaves.view(np.uint8).reshape(cap, -1)), "a kept leaf is no leaf"
        out["leaves"] = _b(np.int32(len(leaves)))
    return out


def test_search_gather():
    """n = 5, S = 32, leaf_cap one less than the leaves produced (rows at or past leaf_cap
    are not written: the guard behind d_leaves sees an overrun)."""
    small, big = _positions(5, 60, finished=False), _positions(9, 61, finished=False)
    p = device.search_params(32, 1.6, 0.05, 0.2, SEED, gather_leaves=True)
    pbig = device.search_params(64, 1.6, 0.05, 0.2, SEED, gather_leaves=True)
    gids = list(range(100, 105))
    _, _, _, every = device.search(small, gids, p, leaf_cap=5 * 33)
    cap = len(every) - 1
    assert cap > 5

    def case(mem, _):
        return _search_out(*device.search(small, gids, p, want_trees=True, leaf_cap=cap), every, cap)

    def larger(mem):
        device.search(big, list(range(200, 209)), pbig, want_trees=True, leaf_cap=9 * 65)

    _four_fills(case, larger)


def test_plan_search():
    small, big = _positions(4, 70, finished=False), _positions(6, 71, finished=False)
    p = device.search_params(16, 1.6, 0.05, 0.2, SEED, planner_steps=2, gather_leaves=True)
    pbig = device.search_params(32, 1.6, 0.05, 0.2, SEED, planner_steps=2, gather_leaves=True)
    pp = _lib.planner_params("medium")

    def case(mem, _):
        gnw = device.GNWeights(_gn_blob())
        return _search_out(*device.plan_search(small, [7, 8, 9, 10], p, pp, gnw, want_trees=True, leaf_cap=4 * 17),
                           None, 0)

    def larger(mem):
        device.plan_search(big, list(range(20, 26)), pbig, pp, device.GNWeights(_gn_blob()), want_trees=True,
                           leaf_cap=6 * 33)

    _four_fills(case, larger)


# ---------------------------------------------------------------- gz_puct_search, the step API, reroot
def _puct_tree_bytes(trees):
    for t in trees:  # scalars next to the arrays
        for k in ("n_nodes", "n_evals", "main_draws", "move"):
            t[k] = np.int32(t[k])
    return _tree_bytes(trees)


@pytest.mark.parametrize("K,noise", [(1, True), (4, False)])
def test_puct_search(K, noise):
    """n = 6 (one board over, one with three empty cells: terminal nodes, whose prior rows no
    evaluation writes), S = 24; the leftover run follows n = 10, S = 48."""
    small, big = _positions(6, 80), _positions(10, 81)
    alpha = 0.3 if noise else None

    def run(st, S, base):
        w = device.PVWeights(_pv_blob(), "f16x3")
        p = device.puct_params(S, 1.6, 4, SEED, "f16x3", dirichlet_alpha=alpha, leaves_per_round=K)
        mv, vis, q, trees = device.puct_search(st, list(range(base, base + len(st))), p, w, want_trees=True)
        assert mv[4] == -1 and not vis[4].any() and all(int(v.sum()) == S for g, v in enumerate(vis) if g != 4)
        assert any((t["term"] != 0).any() for t in trees)
        return {"moves": _b(mv), "visits": _b(vis), "root_q": _b(q), "trees": _puct_tree_bytes(trees)}

    _four_fills(lambda mem, _: run(small, 24, 300), lambda mem: (run(big, 48, 400), None)[1])


def _step_search(mem, st_states, S, base, K, noise):
    """begin / select / backup / remaining / finish / trees with the forward as the caller's
    evaluator, then a re-root (unbatched only) and one more round."""
    n = len(st_states)
    w = device.PVWeights(_pv_blob(), "f16x3")
    p = device.puct_params(S, 1.6, 4, SEED, "f16x3", dirichlet_alpha=0.3 if noise else None, leaves_per_round=K)
    st = device.PuctStepper(st_states, list(range(base, base + n)), p)
    rows = st.rows
    d_probs = mem.torch.empty(rows * 225, dtype=torch.float32, device="cuda")
    d_prior = mem.torch.empty(rows * 225, dtype=torch.float64, device="cuda")

    def evaluate():
        _, d_value, _ = device.pv_forward_dev(w, st.d_leaves, rows, d_probs=d_probs, d_prior=d_prior)
        st.backup(d_prior, d_value)

    out = {}
    evaluate()
    rounds = 0
    while st.remaining().any():
        st.select()
        if rounds == 1:
            lv, act = st.leaves()
            out["round1.leaves"], out["round1.active"] = _b(lv), _b(act)
        evaluate()
        rounds += 1
        assert rounds <= S + 1
    out["rounds"] = _b(np.int32(rounds))
    mv, vis, q = st.finish()
    out["moves"], out["visits"], out["root_q"] = _b(mv), _b(vis), _b(q)
    out["trees"] = _puct_tree_bytes(st.trees())
    if K == 1:
        # moves -1 (keep), the move chosen (it has a child) and an empty cell without a child
        nxt = []
        for g in range(n):
            free = np.flatnonzero((boards.words_to_cells(st_states["black"][g], st_states["white"][g]) == 0)
                                  & (vis[g] == 0))
            nxt.append(-1 if (g % 3 == 0 or mv[g] < 0) else int(mv[g]) if g % 3 == 1 else int(free[-1]))
        rem = st.reroot(nxt)
        lv, act = st.leaves()
        out["reroot.remaining"], out["reroot.leaves"], out["reroot.active"] = _b(rem), _b(lv), _b(act)
        evaluate()  # (a fresh root has no prior row until its evaluation is backed up)
        st.select()
        evaluate()
        out["reroot.remaining2"] = _b(st.remaining())
        out["reroot.trees"] = _puct_tree_bytes(st.trees())
    return out


@pytest.mark.parametrize("K,noise", [(1, False), (4, True)])
def test_puct_step_api_and_reroot(K, noise):
    small, big = _positions(6, 80), _positions(10, 81)
    _four_fills(lambda mem, _: _step_search(mem, small, 24, 300, K, noise),
                lambda mem: (_step_search(mem, big, 48, 400, K, noise), None)[1])


def test_puct_root_noise():
    """d_eta: the zeros at stones and the all-zero row of a full board are stores of the kernel."""
    st = np.concatenate([_positions(6, 90), boards.make_states(_pattern_cells()[None])])

    def case(mem, _):
        eta = device.puct_root_noise(st, list(range(7)), SEED, 0.3)
        assert not eta[6].any() and abs(eta[1].sum() - 1.0) < 1e-12
        return {"eta": _b(eta)}

    _four_fills(case)


# ---------------------------------------------------------------- datasets, gz_puct_cap_full
def test_datasets_and_cap_full():
    from gzero.train import DeviceDataset
    m = 70
    r = np.random.default_rng(SEED + 5)
    rec = np.zeros(m, RECORD_DTYPE)
    rec["black"], rec["white"] = boards.cells_to_words(r.choice(np.array([0, 0, 0, 1, 2], np.int8), size=(m, 225)))
    rec["move"], rec["z"] = r.integers(0, 225, m), r.integers(-1, 2, m)
    rec["game_id"], rec["ply"], rec["player"] = np.arange(m) // 9, np.arange(m) % 9, 1 + np.arange(m) % 2
    vis = r.integers(0, 40, (m, 225)).astype(np.uint16)
    vis[3] = 0  # a row without visits: a row of NaN
    ids = torch.from_numpy(np.concatenate([r.permutation(m + 8 * 35), [3, 3]])).cuda()

    def case(mem, _):
        out = {}
        for name, kw in (("hard", {}), ("soft", {"visits": vis})):
            ds = DeviceDataset(rec, augment_ratio=0.5, fix_labels=True, rng=random.Random(4), **kw)
            for call, res in (("build", ds.materialize()), ("gather", ds.gather(ids))):
                for k, t in zip("xyv", res):
                    out[f"{name}.{call}.{k}"] = _b(t)
        d_rec = torch.from_numpy(rec.view(np.uint8).reshape(-1).copy()).cuda()
        out["cap_full"] = _b(device.cap_full(d_rec, SEED, 0.25))
        return out

    _four_fills(case)


# ---------------------------------------------------------------- the training step
def _train_net():
    net = weights.PolicyValueNet()
    net.load_state_dict(weights.init_state_dict(3))
    return net


def _train_batch(B):
    def make():
        r = np.random.default_rng(SEED + B)
        cells = r.choice(np.array([0, 0, 0, 1, 2], np.int8), size=(B, 225))
        pi = r.multinomial(200, np.ones(225) / 225, size=B).astype(np.float32) / np.float32(200)
        return (torch.from_numpy(boards.planes_from_cells(cells)), torch.from_numpy(r.integers(0, 225, B)),
                torch.from_numpy(r.uniform(-1, 1, (B, 1)).astype(np.float32)), torch.from_numpy(pi))
    return _once(("batch", B), make)


def _saved_maps(ws, B):
    lib = _lib.load()
    out = {}
    t = torch.empty((B, 225, 128), dtype=torch.float32, device="cuda")
    for which in (0, 1, 2, 3, 8):  # a0, h1, a1, h2 and the tower output a2
        _lib.check(lib.gz_sgd_saved(device.ptr(ws), B, which, device.ptr(t), device.stream()), "gz_sgd_saved")
        out[f"saved{which}"] = _b(t)
    return out


def _autograd_step(mem, B):
    from gzero import sgd
    lib = _lib.load()
    x, y, v, _ = _train_batch(B)
    net = copy.deepcopy(_train_net()).cuda().train()
    lg, val = sgd.train_forward(net, x.cuda())
    ws = [a for a in mem.allocations if a.nbytes == lib.gz_sgd_workspace_bytes(B)][-1]
    out = _saved_maps(ws.base, B)
    loss = nn.CrossEntropyLoss()(lg, y.cuda()) + nn.MSELoss()(val, v.cuda())
    loss.backward()
    out.update({"logits": _b(lg), "value": _b(val), "loss": _b(loss)})
    out.update({"grad." + k: _b(p.grad) for k, p in net.named_parameters()})
    out.update({"buf." + k: _b(b) for k, b in net.named_buffers()})
    return out


def _netstep(mem, B, soft):
    from gzero import sgd
    x, y, v, pi = _train_batch(B)
    net = copy.deepcopy(_train_net()).cuda().train()
    step = sgd.NetStep(net)
    loss = step.step(x.cuda(), (pi if soft else y).cuda(), v.cuda(), scale=0.5)
    ws, _, pin, vin, dpin, dvin = step._bufs[B]
    out = _saved_maps(ws, B)
    out.update({"loss": _b(loss), "loss3": _b(step.loss), "grads": _b(step.grads), "pin": _b(pin), "vin": _b(vin),
                "dpin": _b(dpin), "dvin": _b(dvin)})
    out.update({"grad." + k: _b(p.grad) for k, p in net.named_parameters()})
    out.update({"buf." + k: _b(b) for k, b in net.named_buffers()})
    return out


@pytest.mark.parametrize("B", [7, 65])
def test_sgd_forward_backward_autograd(B):
    """B = 7 (one weight-gradient group) and 65 (two); the leftover run follows B = 130 on
    the same workspace, whose per-board scales, BN partials and saved maps then lie
    elsewhere."""
    _four_fills(lambda mem, _: _autograd_step(mem, B), lambda mem: (_autograd_step(mem, 130), None)[1])


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("B", [7, 65])
def test_netstep(B, soft):
    _four_fills(lambda mem, _: _netstep(mem, B, soft), lambda mem: (_netstep(mem, 130, soft), None)[1])


def _fc_loss(mem, B, soft):
    """gz_sgd_fc_loss / _soft on their own, every output and the workspace from the shim."""
    lib = _lib.load()
    g = torch.Generator().manual_seed(SEED + B)
    net = _once("fcnet", lambda: _train_net().cuda())
    fcs = [t.detach() for t in (net.policy_fc.weight, net.policy_fc.bias, net.value_fc1.weight, net.value_fc1.bias,
                                net.value_fc2.weight, net.value_fc2.bias)]
    pin, vin = (torch.randn(B, 450, generator=g) * 0.5).cuda(), (torch.randn(B, 225, generator=g) * 0.5).cuda()
    _, y, v, pi = _train_batch(B)
    new = lambda like: mem.torch.empty(tuple(like.shape), dtype=torch.float32, device="cuda")  # noqa: E731
    grads = [new(t) for t in fcs]
    dpin, dvin, loss = new(pin), new(vin), mem.torch.empty(3, dtype=torch.float32, device="cuda")
    ws = mem.torch.empty(int(lib.gz_sgd_fc_workspace_bytes(B)), dtype=torch.uint8, device="cuda")
    fc, fcg = _lib.SgdFc(*[t.data_ptr() for t in fcs]), _lib.SgdFc(*[t.data_ptr() for t in grads])
    fn, who = (lib.gz_sgd_fc_loss_soft, "gz_sgd_fc_loss_soft") if soft else (lib.gz_sgd_fc_loss, "gz_sgd_fc_loss")
    target = (pi if soft else y).cuda().contiguous()
    vv = v.reshape(B).cuda().contiguous()
    _lib.check(fn(ctypes.byref(fc), B, device.ptr(pin), device.ptr(vin), device.ptr(target), device.ptr(vv), 0.5,
                  device.ptr(dpin), device.ptr(dvin), ctypes.byref(fcg), device.ptr(loss), device.ptr(ws),
                  device.stream()), who)
    torch.cuda.synchronize()
    out = {"loss": _b(loss), "dpin": _b(dpin), "dvin": _b(dvin)}
    out.update({f"grad{i}": _b(t) for i, t in enumerate(grads)})
    return out


@pytest.mark.parametrize("soft", [False, True])
@pytest.mark.parametrize("B", [7, 65])
def test_sgd_fc_loss(B, soft):
    _four_fills(lambda mem, _: _fc_loss(mem, B, soft), lambda mem: (_fc_loss(mem, 130, soft), None)[1])


def test_adam_step():
    """Two clipped steps on the net's parameter shapes: parameters, both moments, the
    clipped gradients and last_norm (the norm partials live in the workspace)."""
    from gzero.optim import DeviceAdam

    def case(mem, _):
        net = copy.deepcopy(_train_net()).cuda()
        g = torch.Generator().manual_seed(SEED)
        for p in net.parameters():
            p.grad = (torch.randn(p.shape, generator=g) * 0.1).cuda()
        opt = DeviceAdam(net.parameters(), lr=1e-3, weight_decay=1e-4)
        out = {}
        for k in range(2):
            opt.step(max_norm=0.8)
            out[f"norm{k}"] = _b(opt.last_norm)
        for name, p in net.named_parameters():
            out["p." + name], out["g." + name] = _b(p), _b(p.grad)
            out["m." + name], out["v." + name] = _b(opt.state[p]["exp_avg"]), _b(opt.state[p]["exp_avg_sq"])
        return out

    out = _four_fills(case)
    assert np.frombuffer(out["norm0"], np.float32)[0] > 0.8


# ---------------------------------------------------------------- the engines
def _engine_views(eng, out, tag):
    """Records (with their visit rows on a PUCT engine) as a multiset, the counters."""
    c = eng.counters()
    out[tag + ".counters"] = _b(np.asarray(c))
    recs = eng.records()
    cols = [recs] + ([eng.visits()] if eng.search == "puct" else [])
    out[tag + ".records"] = _b(np.int32(len(recs))) + _b(_rows_sorted(*cols))


def _slot_views(eng, out):
    """Per-slot views by game id (a compaction permutes the slots)."""
    st, gids = eng.boards()
    out["boards"] = _b(_rows_sorted(gids, st, eng.draws()))


def _play(eng, out, plies_per_step, each=None):
    """Steps until the first step in which a game ended (a game is over after 200 plies at
    the latest, so that step exists), and one more: records and visit rows are compared,
    and the last step runs on buffers that finished games and restarts have used."""
    done, k, last = 0, 0, None
    while last is None or k <= last + 1:
        eng.step()
        _engine_views(eng, out, f"step{k}")
        done += int(eng.counters()["games"])
        if each is not None:
            each(k)
        if done and last is None:
            last = k
        k += 1
        assert k * plies_per_step <= 2 * _lib.GZ_MAX_GAME_PLIES + plies_per_step, "no game ended"
    out["steps"] = _b(np.int32(k))


def test_selfplay_engine_fused_tree():
    """32 slots, S = 16, steps of 3 plies with the incremental forward of every node, until a
    game has ended: the engine's own earlier steps are the leftover of every later one."""
    from gzero.selfplay import SelfPlayEngine

    def case(mem, _):
        w = device.PVWeights(_pv_blob(), "f16x3")
        eng = SelfPlayEngine(n_slots=32, num_simulations=16, seed=SEED, pv_weights=w, pv_mode="tree",
                             plies_per_step=3, beta=0.2)
        out, seen = {}, []

        def each(k):
            out[f"step{k}.tree_stats"] = _b(np.asarray(eng.tree_stats(), np.int32))
            n = int(eng.counters()["leaves"])
            assert n <= eng.leaf_cap
            # (plies 0-5 are opening moves without a search: no leaves; else the outputs of
            # every second step)
            if n == 0 or k % 2:
                return
            seen.append(n)
            meta = eng.d_meta[:n].cpu().numpy()
            kind = np.where(meta >= 0, 0, meta).astype(np.int32)  # (a parent's index is a position in this run's order)
            out[f"step{k}.leaves"] = _b(np.int32(n)) + _b(_rows_sorted(
                eng.d_leaves[: n * 16].view(n, 16), kind.reshape(n, 1), eng.d_logits[: n * 225].view(n, 225),
                eng.d_value[:n].view(n, 1), eng.d_probs[: n * 225].view(n, 225), eng.d_prior[: n * 225].view(n, 225)))

        _play(eng, out, 3, each)
        assert seen, "no step's forward outputs were compared"
        _slot_views(eng, out)
        return out

    _four_fills(case)


def test_selfplay_engine_planner():
    """8 slots, S = 16, planner_steps = 2, one ply per step until a game has ended."""
    from gzero.selfplay import SelfPlayEngine

    def case(mem, _):
        w = device.PVWeights(_pv_blob(), "f16x3")
        eng = SelfPlayEngine(n_slots=8, num_simulations=16, seed=SEED, pv_weights=w, planner_steps=2,
                             gn_weights=device.GNWeights(_gn_blob()), beta=0.2, plies_per_step=2)
        out = {}
        _play(eng, out, 2)
        n = int(eng.counters()["leaves"])
        out["leaves"] = _b(np.int32(n)) + _b(_rows_sorted(
            eng.d_leaves[: n * 16].view(n, 16), eng.d_logits[: n * 225].view(n, 225), eng.d_value[:n].view(n, 1)))
        _slot_views(eng, out)
        return out

    _four_fills(case)


PUCT_ENGINES = {
    "lock_step": dict(),
    "tree_reuse": dict(tree_reuse=True, dirichlet_alpha=0.3),
    "leaf_batch": dict(leaves_per_round=4),
    "compact": dict(game_id_end=24, compact_slots=True),
    "compact_reuse": dict(game_id_end=24, compact_slots=True, tree_reuse=True),
    "playout_cap": dict(fast_simulations=4, full_prob=0.25, tree_reuse=True),
}


@pytest.mark.parametrize("mode", sorted(PUCT_ENGINES))
def test_selfplay_engine_puct(mode):
    """16 slots, S = 16, the move sampled from the visits on every ply so that games differ;
    steps of 4 plies (68 rounds with tree reuse) until a game has ended, compacting after
    every step where the engine can."""
    from gzero.selfplay import SelfPlayEngine
    kw = PUCT_ENGINES[mode]

    def case(mem, _):
        w = device.PVWeights(_pv_blob(), "f16x3")
        eng = SelfPlayEngine(n_slots=16, num_simulations=16, seed=SEED, pv_weights=w, search="puct", temp_plies=200,
                             rounds_per_step=68 if kw.get("tree_reuse") else None, plies_per_step=4, **kw)
        out = {}

        def each(k):
            if eng.compact_slots:
                eng.n_active = int(eng.compact().item())
                out[f"step{k}.n_active"] = _b(np.int32(eng.n_active))

        _play(eng, out, 4, each)
        assert len(eng.records()) > 0 or any(len(v) > 4 for name, v in out.items() if name.endswith(".records"))
        _slot_views(eng, out)
        return out

    _four_fills(case)


def test_puct_match():
    """16 games, S = 16, weights 0 (f16x3) against 1 (f16), in steps of 4 plies until 4 games
    have ended (200 plies at the latest)."""
    from gzero import arena

    def case(mem, _):
        a, b = device.PVWeights(_pv_blob(0), "f16x3"), device.PVWeights(_pv_blob(1), "f16")
        match = arena.PuctMatch(a, b, 16, num_simulations=16, temp_plies=200, seed=SEED, dirichlet_alpha=0.3)
        plies = 0
        while match.games_done < 4 and plies < _lib.GZ_MAX_GAME_PLIES:
            match.step(4)
            plies += 4
        recs, vis = match.records()
        assert match.games_done >= 4 and len(recs) > 0
        st, gids = match.boards()
        return {"records": _b(np.int32(len(recs))) + _b(recs) + _b(vis), "tally": _b(match.d_tally),
                "results": _b(match.results()), "boards": _b(_rows_sorted(gids, st)),
                "moves": _b(np.int64(match.moves_played)), "plies": _b(np.int32(plies))}

    _four_fills(case)


def test_selfplay_compact_direct():
    """gz_selfplay_compact into a poisoned d_dst: every slot of d_dst is written (headers
    compared: the record area behind a header is scratch), *d_n_active too."""
    from gzero.selfplay import SelfPlayEngine
    lib = _lib.load()
    idle = [1, 4, 5]

    def case(mem, _):
        eng = SelfPlayEngine(n_slots=8, num_simulations=16, seed=SEED, game_id_end=1000)
        eng.advance(3)
        stride = eng.d_slots.numel() // 8
        hdr = eng.d_slots.view(torch.int64).view(8, stride // 8)
        hdr[idle, 88 // 8] = 0  # SlotHeader.game_id_end: these slots' games are done
        d_dst = mem.torch.empty(eng.d_slots.numel(), dtype=torch.uint8, device="cuda")
        d_n = mem.torch.empty(1, dtype=torch.int32, device="cuda")
        ws = mem.torch.empty(lib.gz_selfplay_compact_workspace_bytes(8), dtype=torch.uint8, device="cuda")
        _lib.check(lib.gz_selfplay_compact(device.ptr(eng.d_slots), 8, device.ptr(d_dst), device.ptr(d_n),
                                           device.ptr(ws), device.stream()), "gz_selfplay_compact")
        torch.cuda.synchronize()
        assert int(d_n.item()) == 5
        got = d_dst.view(8, stride)[:, :128].cpu().numpy()
        src = eng.d_slots.view(8, stride)[:, :128].cpu().numpy()
        order = [s for s in range(8) if s not in idle] + idle
        assert np.array_equal(got, src[order])
        return {"headers": _b(got), "n_active": _b(d_n)}

    _four_fills(case)
