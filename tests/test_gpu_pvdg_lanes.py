"""pv_dg_kernel's lane-channel mapping (csrc/gz_pvdg.hip: a lane owns the 8 channels of
one 16-byte slot, 32 np + 8 q + 4 n + r, so the D squares, the patches, the LDS images
and the skip / x0 loads are 16-byte accesses; the weight fragments are picked per lane
to match) and its row-class order (csrc/gz_dgclass.h).

One root of 20 stones; children on the four corners, four edge midpoints, the centre
and one cell at each distance 1..5 from an edge (every radius of the D squares clips),
fed in lists of 1, 5, 6, 7 and 13 children (ragged last chunks, chunks shorter than
an XCD's share of the list) and of 56 (7 per XCD: a full chunk of 6 and a ragged one).
The first and the last child of a list carry three grandchildren each: their patches are
written by the 16-byte stores and read by pv_sib_kernel.

Against the full f16x3 forward of the same boards (the additions in another order, the x2
head sums grouped by other channels per lane): logits and value within 2e-5, softmax and
the masked prior within 1e-6, the root bit for bit, and the list counts as expected.
"""
import numpy as np
import pytest

from conftest import SEED
from gzero import weights
from test_gpu_pvinc import _close, _root_family, _rows

pytestmark = pytest.mark.gpu

CORNERS = [0, 14, 210, 224]
EDGE_MIDS = [7, 105, 119, 217]
CENTRE = [112]
# (row, col): distance 1 from the top, 2 from the left, 3 from the bottom, 4 from the right, 5 from the top
NEAR_EDGE = [1 * 15 + 5, 6 * 15 + 2, 11 * 15 + 9, 8 * 15 + 10, 5 * 15 + 7]
SPECIAL = CORNERS + EDGE_MIDS + CENTRE + NEAR_EDGE
# (list length, first child): together the short lists cover every special cell
CASES = [(1, 13), (5, 0), (6, 5), (7, 7), (13, 0), (56, 0)]


@pytest.fixture(scope="module")
def pvw():
    from gzero.device import PVWeights
    return PVWeights(weights.pack_pv_weights(weights.init_state_dict(0)), precision="f16x3")


@pytest.fixture(scope="module")
def family(pvw):
    """The root, 56 children (the special cells first) and three grandchildren of every
    special child (the nearest, the middle and the farthest empty cell by Chebyshev
    distance from its stone), with the full forward of them all, computed once."""
    from gzero import device
    rng = np.random.default_rng(SEED + 11)
    for _ in range(1000):  # a 20-stone root that leaves the special cells empty
        root, kids = _root_family(rng, 20)
        if not root[SPECIAL].any():
            break
    assert not root[SPECIAL].any()
    mover = 1  # 20 stones: black to move
    empties = np.flatnonzero(root == 0)
    kid_of = {int(c): kids[i] for i, c in enumerate(empties)}
    assert all(kid_of[c][c] == mover for c in SPECIAL)
    cells_order = SPECIAL + [int(c) for c in empties if c not in SPECIAL][:56 - len(SPECIAL)]
    boards_ = [root] + [kid_of[c] for c in cells_order]
    grand = {}
    for c in SPECIAL:
        k = kid_of[c]
        e = np.flatnonzero(k == 0)
        dist = np.maximum(np.abs(e // 15 - c // 15), np.abs(e % 15 - c % 15))
        e = e[np.argsort(dist, kind="stable")]
        grand[c] = []
        for gc in (e[0], e[len(e) // 2], e[-1]):
            g = k.copy()
            g[gc] = 3 - mover
            grand[c].append(len(boards_))
            boards_.append(g)
    rows = _rows(boards_)
    full = [np.asarray(x).reshape(len(boards_), -1) for x in device.pv_forward(pvw, rows, want_prior=True)[:4]]
    for x in full:
        x.setflags(write=False)
    return rows, full, cells_order, grand


@pytest.mark.parametrize("length,first", CASES)
def test_children_lists_and_patches(pvw, family, length, first):
    from gzero import device
    rows, full, cells_order, grand = family
    kids = list(range(1 + first, 1 + first + length))  # indices into the family's boards
    parents = sorted({kids[0], kids[-1]} & set(range(1, 1 + len(SPECIAL))))
    idx, meta = [0] + kids, [-1] + [0] * length
    for p in parents:
        for g in grand[cells_order[p - 1]]:
            idx.append(g)
            meta.append(idx.index(p))
    tree = device.pv_forward_tree(pvw, rows[idx], meta)
    assert tree[4] == [1, 1, length, 0, 3 * len(parents), len(parents)], tree[4]
    err = _close([x[idx] for x in full], tree, len(idx), exact_rows=[0])
    print(f"{length} children from {first}, {len(parents)} parents:", err)


def test_cases_cover_every_special_cell():
    """(the lists of at most 13 children together place a child on each of the 14 cells)"""
    seen = set()
    for length, first in CASES:
        if length <= 13:
            seen |= set(range(first, first + length))
    assert seen == set(range(len(SPECIAL))) and len(set(SPECIAL)) == 14
