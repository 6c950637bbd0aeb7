// gz_sym.h -- the 8 symmetries of the board for the PUCT search's leaf evaluation (opt-in,
// GZ_PUCT_LEAF_SYM; gz_pv_forward_sym).  tests/puct_sym_ref.py restates it in Python.
//
// t = 2 k + f, k in 0..3 rotations, f in {0, 1}: y = flip^f(rot90^k(x)), np.rot90 (counter-
// clockwise) and then np.flip along the columns -- training._transform_planes' and
// gz_train.hip's aug_source convention.  Cell c' of y holds x[sym_src(t, c')]; a 225-wide
// row o_y computed on y goes back to x's frame as o[c] = o_y[sym_dst(t, c)], sym_dst(t, .)
// the inverse permutation of sym_src(t, .).  t = 0 is the identity.
//
// Which t: a pure function of the seed and the 16 words of the leaf row (black[8],
// white[8]), so a position is evaluated the same way wherever it is met:
//   key = mix64(seed + GOLDEN); for i in 0..7: key = mix64(key ^ (row[i] | row[8 + i] << 32))
//   t   = draw(key, 0x53594D4D) >> 61                                   ("SYMM")
//
// Everything is GZ_HD: the kernels, the host entry point and the stand-alone host test
// (tests/hosttest/sym_main.cpp) compile the same lines.
#pragma once
#include "gz_bitboard.h"

namespace gz {

static constexpr uint32_t GZ_SYM_DRAW = 0x53594D4Du;

GZ_HD int sym_of(uint64_t seed, const uint32_t* row) {
    uint64_t key = mix64(seed + GOLDEN);
    for (int i = 0; i < 8; i++) key = mix64(key ^ ((uint64_t)row[i] | ((uint64_t)row[8 + i] << 32)));
    return (int)(draw(key, GZ_SYM_DRAW) >> 61);
}

// the cell of x that cell (i, j) of y reads: aug_source(i, j, k, f)
GZ_HD int sym_src(int t, int cell) {
    const int k = t >> 1, f = t & 1;
    const int i = cell / GZ_N;
    int j = cell % GZ_N;
    if (f) j = GZ_N - 1 - j;
    const int a = (k == 0) ? i : (k == 1) ? j : (k == 2) ? GZ_N - 1 - i : GZ_N - 1 - j;
    const int b = (k == 0) ? j : (k == 1) ? GZ_N - 1 - i : (k == 2) ? GZ_N - 1 - j : i;
    return a * GZ_N + b;
}

// the cell of y that holds cell (a, b) of x: sym_src(t, sym_dst(t, c)) == c
GZ_HD int sym_dst(int t, int cell) {
    const int k = t >> 1, f = t & 1;
    const int a = cell / GZ_N, b = cell % GZ_N;
    const int i = (k == 0) ? a : (k == 1) ? GZ_N - 1 - b : (k == 2) ? GZ_N - 1 - a : b;
    int j = (k == 0) ? b : (k == 1) ? a : (k == 2) ? GZ_N - 1 - b : GZ_N - 1 - a;
    if (f) j = GZ_N - 1 - j;
    return i * GZ_N + j;
}

}  // namespace gz
