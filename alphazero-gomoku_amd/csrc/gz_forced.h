// gz_forced.h -- forced playouts and policy-target pruning at the PUCT search root (opt-in,
// GZ_PUCT_FORCED_PLAYOUTS; KataGo's paper, section 3.2).  tests/puct_forced_ref.py restates
// every line in Python, bit for bit.
//
// Forcing: a root child with n >= 1 visits under a root with T = visits[0] - 1 finished
// simulations is selected ahead of every score while n < forced_min(k, prior, T).  Pruning:
// when the root's visit row is handed out, the child with the most visits keeps its count and
// every other child loses, one at a time and at most (int)forced_min of them, the visits it
// would not hold by PUCT against that child's score; a child left with one visit gets none.
//
// Everything is GZ_HD and uses only + * / and sqrt on doubles, in the order written, so the
// device, the host and CPython round alike.  The unit that includes this header is compiled
// with -ffp-contract=off (no fused multiply-add).  No GPU type is needed: the header stands
// alone in a host program (tests/hosttest/forced_main.cpp).
#pragma once
#include <cstdint>

#ifndef GZ_HD
#if defined(__HIPCC__)
#define GZ_HD __host__ __device__ inline
#else
#define GZ_HD static inline
#endif
#endif

namespace gz {

static constexpr double GZ_FORCED_K_MAX = 16.0;

// forced_k as an argument: finite, in [0, 16] (a NaN fails both)
GZ_HD bool forced_k_ok(double k) { return k >= 0.0 && k <= GZ_FORCED_K_MAX; }

// the playouts a visited root child of prior `prior` is owed after T simulations
GZ_HD double forced_min(double k, double prior, int T) { return __builtin_sqrt((k * prior) * (double)T); }

// the PUCT score of a root child with n >= 1 visits, sq = sqrt((double)visits[0])
GZ_HD double forced_score(double c_puct, double prior, double sq, double q, int n) {
    return q + ((c_puct * prior) * sq) / (1.0 + (double)n);
}

// min(n, (int)f) for f >= 0 (a NaN, from an evaluator's non-finite prior: 0)
GZ_HD int forced_cap(double f, int n) {
    if (f >= (double)n) return n;
    return f > 0.0 ? (int)f : 0;
}

// r: the visits child (prior, W, n >= 1) gives back, T = visits[0] - 1, best = the score of
// the most-visited child.  q is held at W / n while the count falls.
GZ_HD int forced_prune_count(double c_puct, double k, double prior, double sq, int T, double W, int n, double best) {
    const double q = W / (double)n;
    const int m = forced_cap(forced_min(k, prior, T), n);
    int r = 0;
    while (r < m) {
        const double s = forced_score(c_puct, prior, sq, q, n - (r + 1));
        if (s >= best) break;
        r += 1;
    }
    return r;
}

// the count that goes into the row
GZ_HD int forced_kept(int n, int r) {
    const int out = n - r;
    return (r > 0 && out == 1) ? 0 : out;
}

// One row on the host: visits[c] == 0 means no child at c; a child is at an empty cell.
// out may not alias visits.  The device (prune_row, gz_puct.hip) runs the functions above
// with the argmax and the broadcast of `best` across its lanes.
GZ_HD void forced_prune_row(double c_puct, double k, int32_t root_visits, const double* prior, const double* W,
                            const int32_t* visits, int32_t* out, int cells) {
    int best_c = -1, best_n = 0;
    for (int c = 0; c < cells; c++) {
        out[c] = visits[c];
        if (visits[c] > best_n) {
            best_n = visits[c];
            best_c = c;
        }
    }
    if (best_c < 0) return;
    const double sq = __builtin_sqrt((double)root_visits);
    const double best = forced_score(c_puct, prior[best_c], sq, W[best_c] / (double)best_n, best_n);
    for (int c = 0; c < cells; c++) {
        const int n = visits[c];
        if (c == best_c || n < 1) continue;
        out[c] = forced_kept(n, forced_prune_count(c_puct, k, prior[c], sq, root_visits - 1, W[c], n, best));
    }
}

}  // namespace gz
