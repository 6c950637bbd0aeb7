"""gz_pv_tree_workspace_bytes is pure arithmetic on (n, root_cap) and the CU count
(256: the MI355X's, and the fall-back without a device).  The sizes below were recorded
from the library before the workspace layout moved into one function (gz_pvnet.h
tree_layout); they cover the n < 1 and root_cap < 0 clamps, the n / 64 rounding on both
sides of 64 and the bench's own size."""
import pytest

from gzero import _lib

SIZES = {
    (0, 0): 258481152,
    (1, 0): 258481152,
    (1, 1): 260873472,
    (63, 1): 261048064,
    (64, 2): 263443200,
    (65, 2): 263447808,
    (1000, 3): 268501504,
    (5, -1): 258492416,
    (819200, 4096): 12389765632,
}


@pytest.mark.parametrize("shape", sorted(SIZES))
def test_tree_workspace_bytes_pinned(shape):
    L = _lib.load()
    assert L.gz_pv_tree_workspace_bytes(*shape) == SIZES[shape]


def test_negative_root_cap_is_zero():
    L = _lib.load()
    assert L.gz_pv_tree_workspace_bytes(5, -1) == L.gz_pv_tree_workspace_bytes(5, 0)
