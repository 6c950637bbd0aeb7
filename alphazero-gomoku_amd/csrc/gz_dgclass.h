// gz_dgclass.h -- the order of pv_dg_kernel's 36 row classes (gz_pvdg.hip dg_rows_all).
//
// A row of a pass needs the taps TY x TX, each a set of offsets {-1, 0, +1} (bit 0: -1,
// bit 1: 0, bit 2: +1) that is an interval: 6 sets per axis, 36 classes.  The rows are
// counting-sorted by class rank and cut into 16-row tiles; a tile runs the union of its
// rows' taps, so a tile that straddles two classes pays for both -- the less the closer
// the neighbours' tap sets.
//
// Axis order {-1}, {-1,0}, {-1,0,1}, {0,1}, {1}, {0}: nested, each set beside its
// supersets (the union of two neighbours is the larger of them, but for {1} | {0}).
// The x order runs backwards on odd y ranks (a snake), so neighbouring classes differ
// on one axis only -- also across a change of the y set.
// tools/tile_rows_sim.py: 90.9 executed tile-taps per child against 97.5 for the order
// {-1,0,1}, {-1,0}, {-1}, {0,1}, {0}, {1} without the snake (an annealed free permutation
// of the 36 classes: 90.3).
//
// Plain C++ (no HIP include): tests/hosttest/dg_class_main.cpp prints the order on the host.
#pragma once

#ifdef __HIPCC__
#define GZ_DGCLASS_FN __host__ __device__ constexpr
#else
#define GZ_DGCLASS_FN constexpr
#endif

GZ_DGCLASS_FN int dg_set_rank(int b) {
    return b == 1 ? 0 : (b == 3 ? 1 : (b == 7 ? 2 : (b == 6 ? 3 : (b == 4 ? 4 : 5))));
}
GZ_DGCLASS_FN bool dg_set_valid(int b) { return b == 1 || b == 3 || b == 7 || b == 6 || b == 4 || b == 2; }

// class rank (0..35) of the tap sets ty, tx
GZ_DGCLASS_FN int dg_class_rank(int ty, int tx) {
    const int ry = dg_set_rank(ty), rx = dg_set_rank(tx);
    return ry * 6 + ((ry & 1) ? 5 - rx : rx);
}

GZ_DGCLASS_FN bool dg_class_rank_is_permutation() {
    unsigned long long seen = 0;
    for (int ty = 1; ty < 8; ty++)
        for (int tx = 1; tx < 8; tx++) {
            if (!dg_set_valid(ty) || !dg_set_valid(tx)) continue;
            const int k = dg_class_rank(ty, tx);
            if (k < 0 || k >= 36 || ((seen >> k) & 1ull)) return false;
            seen |= 1ull << k;
        }
    return seen == (1ull << 36) - 1ull;
}
static_assert(dg_class_rank_is_permutation(), "the 36 valid (ty, tx) pairs map onto 0..35 exactly once");

#undef GZ_DGCLASS_FN
