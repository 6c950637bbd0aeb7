"""Plain-Python restatement of the PUCT search's leaf symmetry (csrc/gz_sym.h,
csrc/gz_pvsym.hip; GZ_PUCT_LEAF_SYM), the checker of tests/test_puct_sym_cpu.py and
tests/test_gpu_pv_sym.py.  Not a test.

t = 2 k + f: the transformed board is y = flip^f(rot90^k(x)) -- np.rot90, then np.flip
along the columns -- and a 225-wide row computed on y goes back to x's frame by the
inverse.  Both are written with np.rot90 / np.flip on 15 x 15 arrays, not with the
kernels' index arithmetic, so they state the transform independently.

Every PUCT reference (puct_ref.search, puct_batch_ref, puct_reuse_ref, puct_cap_ref,
puct_match_ref) takes an ``evalf(cells, player)``; ``wrap(evalf, seed)`` is the whole
reference of the flag for every mode.
"""
import numpy as np

from gzero import rng

N = 15
SYM_DRAW = 0x53594D4D  # "SYMM"


def pack_row(cells):
    """[16] uint32 words of 225 cells (0 empty, 1 black, 2 white): bit 16 r + c, black[8] then white[8]."""
    row = [0] * 16
    for c, x in enumerate(cells):
        if x:
            b = 16 * (c // N) + c % N
            row[(8 if int(x) == 2 else 0) + (b >> 5)] |= 1 << (b & 31)
    return row


def sym_of(seed, row):
    """The transform 0..7 of a leaf row (16 words): a function of the seed and the position."""
    key = rng.mix64((int(seed) + rng.GOLDEN) & rng.M64)
    for i in range(8):
        key = rng.mix64(key ^ (int(row[i]) | (int(row[8 + i]) << 32)))
    return rng.draw(key, SYM_DRAW) >> 61


def transform_cells(cells, t):
    """The 225 cells of y = flip^f(rot90^k(x))."""
    k, f = t >> 1, t & 1
    y = np.rot90(np.asarray(cells).reshape(N, N), k=k)
    if f:
        y = np.flip(y, axis=1)
    return np.ascontiguousarray(y).reshape(225)


def map_back(row225, t):
    """A 225-wide row computed on y, in x's frame."""
    k, f = t >> 1, t & 1
    o = np.asarray(row225).reshape(N, N)
    if f:
        o = np.flip(o, axis=1)
    return np.ascontiguousarray(np.rot90(o, k=-k)).reshape(225)


def wrap(evalf, seed):
    """evalf under the leaf symmetry: the transform of the position, evalf on the
    transformed board, the prior mapped back; the value as it is."""

    def evalf_sym(cells, player):
        cells = tuple(int(x) for x in cells)
        t = sym_of(seed, pack_row(cells))
        prior, value = evalf(tuple(int(x) for x in transform_cells(cells, t)), player)
        return [float(x) for x in map_back(np.asarray(prior, np.float64), t)], value

    return evalf_sym
