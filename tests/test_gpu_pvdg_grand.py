"""Grandchildren on the delta form of pv_dg_kernel (csrc/gz_pvdg.hip, the OVERLAY
instantiation): a grandchild G = parent C + a stone at m2, C = root R + a stone at m1, is
evaluated as a delta of C.  C's pre-ReLU values are its patch (fp32, written by the
children's launch) inside its changed square -- radius L + 2 around m1 at the output of
layer L -- and the root's elsewhere, so the kernel can go wrong where G's square (the same
radius around m2) meets C's: they overlap iff the Chebyshev distance d(m1, m2) <= 2 (L + 2),
boundaries at d = 4, 6, 8, 10, and conv0's reference x0 flips at d = 2.

Two roots of 20 stones.  Every board of every case below goes through ONE full f16x3
forward (the module's reference); each case is a call of device.pv_forward_tree on a
subset: logits and value within DELTA_TOL = 2e-5, softmax and the masked prior within
1e-6, the roots bit for bit, the list counts as expected -- the children's rows of the same
calls included (their patch stores are what the grandchildren read).

A list of grandchildren is cut into 8 shares (one per XCD) before it is cut into chunks of
6, so a chunk is full only from 41 entries up: the lists of 1, 5, 6, 7 and 13 run ragged
chunks, the list of 56 (8 parents x 7) gives each share one parent's full chunk and a
ragged one, and the list of 48 (48 parents, the two roots' alternating in threes) chunks of
six grandchildren with six parents under two roots.
"""
import numpy as np
import pytest

from conftest import SEED
from gzero import weights
from test_gpu_pvinc import _close, _rows

pytestmark = pytest.mark.gpu

BLACK, WHITE = 1, 2  # 20 stones: black moves (the parents' stones), then white (the grandchildren's)


def rc(r, c):
    return r * 15 + c


# ---- the cases: (root, parent cell m1, grandchild cells m2) ----
# every distance 1..7 from the centre and 1..11 from (3, 3) (no cell is 11 from the centre
# of a 15 x 15 board), along a row, a column and a diagonal; d = 11: no square overlaps
CENTRE, OFF = rc(7, 7), rc(3, 3)
DIST = [(0, CENTRE, [rc(7, 7 + d) for d in range(1, 8)] + [rc(7 + d, 7) for d in range(1, 8)] +
         [rc(7 + d, 7 + d) for d in range(1, 8)]),
        (0, OFF, [rc(3, 3 + d) for d in range(1, 12)] + [rc(3 + d, 3) for d in range(1, 12)] +
         [rc(3 + d, 3 + d) for d in range(1, 12)])]
# parent and grandchild both within two cells of a corner / of an edge midpoint
CLIP = [(0, rc(0, 0), [rc(1, 1), rc(2, 2), rc(0, 2), rc(2, 1)]),
        (0, rc(1, 2), [rc(0, 0), rc(2, 0), rc(0, 1)]),
        (0, rc(14, 14), [rc(13, 13), rc(12, 14), rc(14, 12)]),
        (0, rc(13, 0), [rc(14, 0), rc(12, 2), rc(14, 2)]),
        (0, rc(1, 13), [rc(0, 14), rc(2, 12), rc(0, 12)]),
        (0, rc(0, 7), [rc(1, 7), rc(2, 8), rc(0, 5), rc(2, 6)]),
        (0, rc(2, 6), [rc(0, 7), rc(1, 8), rc(0, 5)]),
        (0, rc(7, 14), [rc(7, 12), rc(9, 13), rc(5, 14)]),
        (0, rc(14, 8), [rc(14, 7), rc(12, 6), rc(13, 9)]),
        (0, rc(6, 1), [rc(7, 0), rc(8, 2), rc(5, 0)])]
# lists of 1, 5, 6, 7 and 13 grandchildren (parents of root 1, cells of rows 5 / 9)
P_A, P_B = rc(5, 5), rc(9, 9)
G_A = [rc(5, 6), rc(4, 4), rc(5, 9), rc(8, 5), rc(5, 11), rc(11, 5), rc(1, 5)]
G_B = [rc(9, 8), rc(10, 10), rc(9, 5), rc(6, 9), rc(9, 2), rc(2, 9)]
SHORT = {1: [(1, P_A, G_A[:1])], 5: [(1, P_A, G_A[:5])], 6: [(1, P_A, G_A[:6])], 7: [(1, P_A, G_A)],
         13: [(1, P_A, G_A), (1, P_B, G_B)]}
# 56: 8 parents x 7 grandchildren at distances 1..7 (row 5 + k of root 1, both squares clip on the left)
LIST56 = [(1, rc(4 + k, 1), [rc(4 + k, 1 + d) for d in range(1, 8)]) for k in range(8)]
# 48 parents with one grandchild each, leaves ordered A A A B B B ...: parent (r, c) on the
# even rows, its grandchild two columns on (d = 2 ... 4 by row)
LIST48 = []
for _k in range(48):
    _blk, _j = divmod(_k, 3)
    _root = _blk & 1
    _i = (_blk >> 1) * 3 + _j  # 0..23 per root
    _r, _c = 2 * (_i // 4) + 1, 3 * (_i % 4) + 1
    LIST48.append((_root, rc(_r, _c), [rc(_r + (_i % 3), _c + 2 + (_i % 3))]))
# 18 parents with two grandchildren each under one root with root_cap = 1: 11 patch slots
# (the pool of one root map slot)
FALLBACK = [(0, rc(2 * (i // 4) + 1, 3 * (i % 4) + 1),
             [rc(2 * (i // 4) + 2, 3 * (i % 4) + 2), rc(2 * (i // 4) + 2, 3 * (i % 4) + 1)]) for i in range(18)]
ALL = DIST + CLIP + sum(SHORT.values(), []) + LIST56 + LIST48 + FALLBACK


@pytest.fixture(scope="module")
def pvw():
    from gzero.device import PVWeights
    return PVWeights(weights.pack_pv_weights(weights.init_state_dict(0)), precision="f16x3")


@pytest.fixture(scope="module")
def family(pvw):
    """Two 20-stone roots that leave every cell of the cases empty, every parent and
    grandchild of the cases, and the full forward of them all, computed once."""
    from gzero import device
    rng = np.random.default_rng(SEED + 21)
    used = [set(), set()]
    for r, m1, m2s in ALL:
        assert m1 not in m2s and len(set(m2s)) == len(m2s) and all(0 <= c < 225 for c in [m1] + m2s)
        used[r] |= {m1, *m2s}
    cells, index = [], {}
    for r in range(2):
        free = np.array([c for c in range(225) if c not in used[r]])
        assert len(free) >= 20
        stones = rng.choice(free, size=20, replace=False)
        root = np.zeros(225, np.int8)
        root[stones[0::2]] = BLACK
        root[stones[1::2]] = WHITE
        index[(r,)] = len(cells)
        cells.append(root)
    for r, m1, m2s in ALL:
        if (r, m1) not in index:
            k = cells[index[(r,)]].copy()
            k[m1] = BLACK
            index[(r, m1)] = len(cells)
            cells.append(k)
        for m2 in m2s:
            if (r, m1, m2) not in index:
                g = cells[index[(r, m1)]].copy()
                g[m2] = WHITE
                index[(r, m1, m2)] = len(cells)
                cells.append(g)
    rows = _rows(cells)
    full = [np.asarray(x).reshape(len(cells), -1) for x in device.pv_forward(pvw, rows, want_prior=True)[:4]]
    for x in full:
        x.setflags(write=False)
    return rows, full, index


def _call(pvw, family, items, root_cap=None):
    """The tree forward of the items' roots, parents (in the items' order) and
    grandchildren: (the family's indices, tree outputs, parents, grandchildren)."""
    from gzero import device
    rows, full, index = family
    roots = sorted({it[0] for it in items})
    idx = [index[(r,)] for r in roots]
    meta = [-1] * len(roots)
    at = {}
    for r, m1, _ in items:
        if (r, m1) not in at:
            at[(r, m1)] = len(idx)
            idx.append(index[(r, m1)])
            meta.append(roots.index(r))
    n_grand = 0
    for r, m1, m2s in items:
        for m2 in m2s:
            idx.append(index[(r, m1, m2)])
            meta.append(at[(r, m1)])
            n_grand += 1
    tree = device.pv_forward_tree(pvw, rows[idx], meta, root_cap=root_cap)
    return idx, tree, len(roots), len(at), n_grand


def _check(pvw, family, items, root_cap=None):
    idx, tree, n_roots, n_par, n_grand = _call(pvw, family, items, root_cap)
    assert tree[4] == [n_roots, n_roots, n_par, 0, n_grand, n_par], tree[4]
    err = _close([x[idx] for x in family[1]], tree, len(idx), exact_rows=range(n_roots))
    print(f"{n_par} parents, {n_grand} grandchildren:", err)


@pytest.mark.parametrize("case", range(len(DIST)))
def test_every_distance_three_directions(pvw, family, case):
    """d(m1, m2) = 1..7 around the centre, 1..11 around (3, 3): row, column, diagonal."""
    _check(pvw, family, [DIST[case]])


def test_clipped_squares(pvw, family):
    """Both stones within two cells of a corner or an edge midpoint: both squares clip,
    the patch row is the unclipped offset from m1."""
    _check(pvw, family, CLIP)


@pytest.mark.parametrize("length", sorted(SHORT))
def test_short_lists(pvw, family, length):
    assert sum(len(it[2]) for it in SHORT[length]) == length
    _check(pvw, family, SHORT[length])


def test_full_and_ragged_chunk_per_parent(pvw, family):
    """56 grandchildren, 7 per parent: each XCD's share is one parent's, a chunk of 6 and one of 1."""
    _check(pvw, family, LIST56)


def test_chunks_of_six_parents_under_two_roots(pvw, family):
    """48 grandchildren of 48 parents, the roots alternating in threes: each share of 6 is
    one chunk with six parents, three under each root (root_cap 5: 59 patch slots)."""
    assert [it[0] for it in LIST48[:6]] == [0, 0, 0, 1, 1, 1] and len({(it[0], it[1]) for it in LIST48}) == 48
    _check(pvw, family, LIST48, root_cap=5)


def test_parents_without_a_patch_slot(pvw, family):
    """18 parents with two grandchildren each, 11 patch slots: both grandchildren of each of
    the seven parents left without one take the full forward, bit for bit; the others the
    delta, within tolerance; one call.  Which parents win a slot is the claim order's, so the
    slotless ones are told by their rows: a parent's two grandchildren go the same way, and
    exactly seven parents have both rows equal to the full forward's."""
    idx, tree, n_roots, n_par, n_grand = _call(pvw, family, FALLBACK, root_cap=1)
    assert tree[4] == [1, 1, 18, 14, 22, 18], tree[4]
    full = [x[idx] for x in family[1]]
    _close(full, tree, len(idx), exact_rows=[0])
    eq = np.ones(len(idx), bool)
    for a, b in zip(full, tree[:4]):
        eq &= np.all(np.asarray(a).reshape(len(idx), -1) == np.asarray(b).reshape(len(idx), -1), axis=1)
    pairs = eq[1 + n_par:].reshape(n_par, 2)  # (_call lists a parent's grandchildren together)
    assert (pairs[:, 0] == pairs[:, 1]).all() and int(pairs.all(axis=1).sum()) == 7, pairs


def test_cases_cover_the_boundaries():
    """(every distance 1..11 in three directions; each overlap boundary d = 2, 4, 6, 8, 10 and d + 1)"""
    def d(a, b):
        return max(abs(a // 15 - b // 15), abs(a % 15 - b % 15))
    for lo, m1, m2s in ((7, CENTRE, DIST[0][2]), (11, OFF, DIST[1][2])):
        ds = [d(m1, m) for m in m2s]
        assert ds == list(range(1, lo + 1)) * 3
        assert {(m // 15 == m1 // 15, m % 15 == m1 % 15) for m in m2s} == {(True, False), (False, True), (False, False)}
    for _, m1, m2s in CLIP:
        near = [rc(0, 0), rc(0, 14), rc(14, 0), rc(14, 14), rc(0, 7), rc(7, 0), rc(7, 14), rc(14, 7)]
        assert any(all(d(c, p) <= 2 for c in [m1] + m2s) for p in near), (m1, m2s)
    assert all(len(it[2]) == 7 for it in LIST56) and len(LIST56) == 8
