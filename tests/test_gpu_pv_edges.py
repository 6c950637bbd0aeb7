"""Row counts, device counts and the prior's other branch in the policy-value forward
(csrc/gz_pvnet.hip; the tree forward of csrc/gz_pvinc.hip / gz_pvdg.hip).

The tower kernels run one board per workgroup per loop turn and keep LDS state across
turns; pv_heads_kernel works in tiles of 64 boards (16-row MFMA tiles; rows past the
count re-read the last board); pv_prior_kernel takes 64 boards per workgroup, 16 per
wave.  Every output element of the full forward is one workgroup's or one MFMA row's
own arithmetic, so a board's outputs must not depend on its row, on its neighbours or
on the boards its workgroup ran before it: the full forward is compared BIT FOR BIT
between launches of different shapes (no tolerance).  The tree forward's incremental
rows depend on the sorted lists' tiling and are compared with test_gpu_pvinc's
DELTA_TOL / 1e-6 (_close), its roots bitwise.  The prior is compared bit for bit with
the oracle's restatement fed the device's own softmax, as
test_gpu_pvnet.test_prior_random_boards_exact_vs_oracle does.
"""
import numpy as np
import pytest
import torch

from conftest import SEED
from gzero import boards, device, weights
from test_gpu_pvinc import _close, _root_family, _rows

pytestmark = pytest.mark.gpu

PRECS = ["fp32", "f16x3"]
EDGE_N = [1, 15, 16, 17, 63, 64, 65]
SENTINEL = 0xA5
NAMES = ("logits", "value", "probs", "prior")

_W = {}


def _pvw(prec, bias=None, cell=112):
    """Init weights (seed 0); bias: policy_fc.bias[cell] set to it."""
    key = (prec, bias)
    if key not in _W:
        sd = weights.init_state_dict(0)
        if bias is not None:
            b = sd["policy_fc.bias"].clone()
            b[cell] = bias
            sd["policy_fc.bias"] = b
        _W[key] = device.PVWeights(weights.pack_pv_weights(sd), precision=prec)
    return _W[key]


def _same(a, b, what=""):
    """Four outputs equal bit for bit."""
    for name, x, y in zip(NAMES, a, b):
        x, y = np.ascontiguousarray(x), np.ascontiguousarray(y)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, name)


def _take(out, idx):
    return tuple(np.asarray(x)[idx] for x in out[:4])


def _mixed_cells(n, seed):
    """Boards of mixed density with the empty board, a board with one empty cell and a
    one-stone board among them (also at rows 63 and 64, the heads' tile edge)."""
    rng = np.random.default_rng(seed)
    fill = rng.uniform(0.0, 0.95, n)
    cells = np.where(rng.random((n, 225)) < fill[:, None], rng.integers(1, 3, (n, 225)), 0).astype(np.int8)
    cells[0] = 0
    cells[1] = rng.integers(1, 3, 225)
    cells[1, 17] = 0
    cells[2] = 0
    cells[2, 112] = 1
    if n > 64:
        cells[63] = cells[1]
        cells[64] = 0
    return cells


_BASE = {}


def _base130(prec):
    """The 130-board launch every small launch is compared with (made once)."""
    if prec not in _BASE:
        rows = _rows(_mixed_cells(130, SEED + 50))
        _BASE[prec] = (rows, device.pv_forward(_pvw(prec), rows, want_prior=True))
    return _BASE[prec]


# ---------------------------------------------------------------- C1
@pytest.mark.parametrize("prec", PRECS)
def test_small_row_counts_bitwise(prec):
    """The first n rows alone, n = 1, 15, 16, 17, 63, 64, 65, equal the first n rows of
    the 130-board launch on all four outputs; so do the first 65 rows in reverse order."""
    rows, out = _base130(prec)
    w = _pvw(prec)
    for n in EDGE_N:
        _same(device.pv_forward(w, rows[:n], want_prior=True), _take(out, slice(0, n)), n)
    rev = device.pv_forward(w, rows[:65][::-1], want_prior=True)
    _same(_take(rev, slice(None, None, -1)), _take(out, slice(0, 65)), "reversed")


# ---------------------------------------------------------------- C2
@pytest.mark.parametrize("prec", PRECS)
def test_no_state_carried_between_a_workgroups_boards(prec):
    """g = the CU count workgroups with stride g: g dense boards, then g + 37 sparse ones,
    so every sparse board runs in a workgroup whose LDS a dense board (or a dense and a
    sparse one) used before.  The sparse rows equal launches in which they come first."""
    g = torch.cuda.get_device_properties(0).multi_processor_count
    rng = np.random.default_rng(SEED + 51)
    dense = np.where(rng.random((g, 225)) < 0.89, rng.integers(1, 3, (g, 225)), 0).astype(np.int8)
    sparse = np.zeros((g + 37, 225), np.int8)
    for i in range(1, g + 37):  # row 0: the empty board
        k = int(rng.integers(0, 4))
        sparse[i, rng.choice(225, k, replace=False)] = rng.integers(1, 3, k)
    sparse[g] = 0  # the empty board as a workgroup's third board too
    rows = _rows(np.concatenate([dense, sparse]))
    w = _pvw(prec)
    out = device.pv_forward(w, rows, want_prior=True)
    assert 150 < (dense != 0).sum(axis=1).mean() < 225
    first = device.pv_forward(w, rows[g:2 * g], want_prior=True)  # one board per workgroup
    _same(_take(out, slice(g, 2 * g)), first, "second boards")
    last = device.pv_forward(w, rows[2 * g:], want_prior=True)
    _same(_take(out, slice(2 * g, 2 * g + 37)), last, "third boards")


# ---------------------------------------------------------------- C3
_FAM = {}


def _family130():
    """One root (30 stones), 41 children, then grandchildren under the first three
    children: 130 rows whose every prefix is a valid tagged list; with the full
    forward of all of them."""
    if not _FAM:
        rng = np.random.default_rng(SEED + 52)
        root, kids = _root_family(rng, 30)
        mover = 1
        cells, meta = [root] + kids[:41], [-1] + [0] * 41
        for p in (1, 2, 3):
            for c in np.flatnonzero(cells[p] == 0)[::6]:
                g = cells[p].copy()
                g[c] = 3 - mover
                cells.append(g)
                meta.append(p)
        cells, meta = cells[:130], meta[:130]
        assert len(cells) == 130 and sum(1 for m in meta if m > 0) > 60
        rows = _rows(cells)
        _FAM["x"] = (rows, np.asarray(meta, np.int32), device.pv_forward(_pvw("f16x3"), rows, want_prior=True))
    return _FAM["x"]


def _tree_prefix_check(tree, full, meta, m):
    if m == 0:
        return
    got = [np.asarray(x).reshape(len(meta), -1)[:m] for x in tree[:4]]
    ref = [np.asarray(x).reshape(len(full[1]), -1)[:m] for x in full[:4]]
    _close(ref, got, m, np.flatnonzero(meta[:m] == -1))


def test_tree_forward_small_row_counts():
    """gz_pv_forward_tree at the same row counts: children and grandchildren within
    DELTA_TOL of the full forward, the root bitwise, every row classified."""
    rows, meta, full = _family130()
    w = _pvw("f16x3")
    for n in EDGE_N + [130]:
        tree = device.pv_forward_tree(w, rows[:n], meta[:n])
        st = tree[4]
        kids, grand = int((meta[:n] == 0).sum()), int((meta[:n] > 0).sum())
        assert st[:5] == [1, 1, kids, 0, grand], (n, st)
        _tree_prefix_check(tree, full, meta[:n], n)


# ---------------------------------------------------------------- C4
COUNTS = [0, 1, 63, 64, 65, 100, 107]


@pytest.mark.parametrize("prec", PRECS)
def test_device_counts(prec):
    """d_count of 0, 1, around the 64-row tile edge, n and above n, with capacity n = 100:
    rows below min(count, n) equal the plain forward bit for bit, and every element of
    logits, value, probs and prior past that keeps its sentinel bytes.  A count of 0
    returns GZ_OK (pv_forward_dev raises otherwise) and writes nothing."""
    rows, _ = _base130(prec)
    n = 100
    w = _pvw(prec)
    out = device.pv_forward(w, rows[:n], want_prior=True)  # the plain forward of the same rows
    d_b =torch.from_numpy(np.ascontiguousarray(rows[:n]).view(np.int32).copy()).cuda()
    assert (rows[:n] != 0).any(axis=1).sum() >= n - 2  # nonzero boards (but the empty ones of the mix)
    for count in COUNTS:
        bufs = [torch.empty(n * 225, dtype=torch.float32, device="cuda"),
                torch.empty(n, dtype=torch.float32, device="cuda"),
                torch.empty(n * 225, dtype=torch.float32, device="cuda"),
                torch.empty(n * 225, dtype=torch.float64, device="cuda")]
        for t in bufs:
            t.view(torch.uint8).fill_(SENTINEL)
        d_cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
        device.pv_forward_dev(w, d_b, n, d_count=d_cnt, d_logits=bufs[0], d_value=bufs[1], d_probs=bufs[2],
                              d_prior=bufs[3])
        torch.cuda.synchronize()
        m = min(count, n)
        for name, t, ref in zip(NAMES, bufs, out):
            got = t.cpu().numpy().reshape(n, -1)
            want = np.asarray(ref).reshape(n, -1)[:m]
            assert got[:m].tobytes() == want.tobytes(), (count, name)
            assert (np.ascontiguousarray(got[m:]).view(np.uint8) == SENTINEL).all(), (count, name)


def test_device_counts_tree_forward():
    """The same counts through gz_pv_forward_tree (device.pv_forward_tree's d_count: the
    outputs start as NaN): incremental rows within DELTA_TOL, the root bitwise, nothing
    written past the count."""
    rows, meta, full = _family130()
    n = 100
    w = _pvw("f16x3")
    nan32 = torch.full((1,), float("nan"), dtype=torch.float32).numpy().view(np.uint32)[0]
    nan64 = torch.full((1,), float("nan"), dtype=torch.float64).numpy().view(np.uint64)[0]
    for count in COUNTS:
        tree = device.pv_forward_tree(w, rows[:n], meta[:n], d_count=count)
        m = min(count, n)
        st = tree[4]
        assert st[1] + st[2] + st[3] + st[4] == m, (count, st)
        _tree_prefix_check(tree, full, meta[:n], m)
        for name, x, bits, pat in zip(NAMES, tree[:4], (np.uint32, np.uint32, np.uint32, np.uint64),
                                      (nan32, nan32, nan32, nan64)):
            past = np.ascontiguousarray(np.asarray(x).reshape(n, -1)[m:])
            assert (past.view(bits) == pat).all(), (count, name)


# ---------------------------------------------------------------- C5
CELL = 112


def _prior_boards():
    """Two root families in one tagged list: root 0 has CELL empty (one of its children
    puts a stone there), root 1 has a stone on CELL (so have all its children)."""
    rng = np.random.default_rng(SEED + 53)
    cells, meta = [], []
    for want_stone in (False, True):
        while True:
            root, kids = _root_family(rng, 35 if want_stone else 20)
            if (root[CELL] != 0) == want_stone:
                break
        r = len(cells)
        on_cell = [k for k in kids if k[CELL] != root[CELL]]
        pick = kids[::9] + on_cell
        cells += [root] + pick
        meta += [-1] + [r] * len(pick)
    # and boards that are no one's children: dense ones, and a board whose only empty cell is CELL
    for fill in (0.5, 0.9):
        for stone in (0, 1):
            c = np.where(rng.random(225) < fill, rng.integers(1, 3, 225), 0).astype(np.int8)
            c[CELL] = stone
            cells.append(c)
            meta.append(-2)
    c = rng.integers(1, 3, 225).astype(np.int8)
    c[CELL] = 0
    cells.append(c)
    meta.append(-2)
    return np.asarray(cells, np.int8), np.asarray(meta, np.int32)


def _check_prior(oracle, out, cells, bias, what):
    _, _, probs, prior = out[:4]
    sums = []
    for i, cl in enumerate(cells):
        empty = cl == 0
        assert (prior[i][~empty] == 0.0).all(), (what, i)
        assert prior[i][empty].tobytes() == oracle.prior(probs[i], cl).tobytes(), (what, i)
        s = oracle.np_pairwise_sum([float(x) for x in probs[i][empty]])
        if cl[CELL] != 0:  # the mass sits on an occupied cell
            sums.append(s)
            if s > 0:
                assert abs(oracle.np_pairwise_sum(prior[i][empty]) - 1.0) < 1e-12, (what, i)
            else:  # the raw softmax, here all zeros
                assert not prior[i].any() and not probs[i][empty].any(), (what, i)
        else:  # the normal branch, one cell near 1
            assert probs[i][CELL] > 0.999999 and abs(prior[i][CELL] - 1.0) < 1e-6, (what, i)
    print(f"{what}, bias +{bias}: empty cells' softmax sum on the boards with a stone on the cell: "
          f"min {min(sums):.3e} max {max(sums):.3e}")
    return sums


@pytest.mark.parametrize("prec", PRECS)
def test_prior_when_the_empty_cells_hold_no_mass(oracle, prec):
    """policy_fc.bias[c] = +200: on a board with a stone on c every empty cell's float32
    softmax is exactly 0, their float64 sum is not positive and the prior is the raw
    softmax (v = s > 0 ? x / s : x, ai_agent.py:579): 0 everywhere, the oracle's bit for
    bit.  With c empty it is the normal branch with one cell near 1.  +95 and +80: the
    empty cells keep a tiny mass (exp(-95) is below float32's normal range, exp(-80) is
    not) and the prior is renormalised, bit for bit the oracle's fed the device's
    softmax.  Through the full forward and (f16x3) the tree forward.
    (+95 is the case that found the softmax flushing denormals to 0 where the reference's
    np.exp keeps them -- an all-zero prior instead of a renormalised one; see
    softmax_exp in csrc/gz_pvnet.hip and DESIGN.md 3.3.)"""
    cells, meta = _prior_boards()
    rows = _rows(cells)
    assert (cells[:, CELL] != 0).sum() >= 8 and (cells[:, CELL] == 0).sum() >= 8
    for bias in (200.0, 95.0, 80.0):
        w = _pvw(prec, bias)
        runs = [("full", device.pv_forward(w, rows, want_prior=True))]
        if prec == "f16x3":
            tree = device.pv_forward_tree(w, rows, meta)
            assert tree[4][2] > 0, tree[4]
            runs.append(("tree", tree))
        for what, out in runs:
            sums = _check_prior(oracle, out, cells, bias, f"{prec} {what}")
            if bias == 200.0:
                assert max(sums) == 0.0, sums
            else:
                assert 0.0 < min(sums) and max(sums) < 1e-25, sums  # tiny but positive
