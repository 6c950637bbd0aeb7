// gz_gumbel.h -- the Gumbel root with sequential halving of the PUCT search (opt-in,
// GZ_PUCT_GUMBEL; "Policy improvement by planning with Gumbel", Danihelka et al., ICLR 2022).
// tests/puct_gumbel_ref.py restates every line in Python, bit for bit.
//
// Root preparation (once per root, when node 0's evaluation is stored).  E: the root's empty
// cells.  A cell of E is ok when its prior is normal and finite; with no ok cell every cell of
// E is ok with logit 0.0, else logit(c) = gz_log(prior[c]).  Cell c owns draw c of the
// (seed, game, ply, GZ_GUMBEL_SIM) stream: g(c) = gumbel_scale * (-gz_log(e)), e = -gz_log(u),
// base(c) = g(c) + logit(c).  The considered set: m = min(max_considered, ok cells) times the
// first maximum of base over the ok cells not yet taken; gs[c] = base(c) there, -infinity
// elsewhere.
// Schedule: gumbel_sequence(m, S)[t] is the visit count the considered child selected at
// simulation t has (sequential halving over ceil(log2 m) phases, in integers).
// Root selection, the move and the policy target: gumbel_score, gumbel_policy_row below.
// q lives in [-1, 1]; there is no min-max rescaling.
//
// Everything is GZ_HD and uses only + - * / on doubles and gz_log / gz_exp (gz_dirichlet.h), in
// the order written, so the device, the host and CPython round alike.  The unit that includes
// this header is compiled with -ffp-contract=off.  No GPU type is needed: the header stands
// alone in a host program (tests/hosttest/gumbel_main.cpp).
#pragma once
#include "gz_dirichlet.h"

namespace gz {

static constexpr int32_t GZ_GUMBEL_SIM = 0x47554D42;  // "GUMB"; simulation streams use sim <= 4095
static constexpr int GZ_GUMBEL_MAX_CONSIDERED = 32;
static constexpr double GZ_GUMBEL_ROW_SCALE = 32767.0;
static constexpr double GZ_GUMBEL_DBL_MIN = 0x1p-1022, GZ_GUMBEL_DBL_MAX = 0x1.fffffffffffffp+1023;

// the arguments: finite and in range (a NaN fails both comparisons)
GZ_HD bool gumbel_args_ok(int max_considered, double c_visit, double c_scale, double gumbel_scale) {
    return max_considered >= 1 && max_considered <= GZ_GUMBEL_MAX_CONSIDERED && c_visit >= 0.0 && c_visit <= 1e4 &&
           c_scale >= 0.0 && c_scale <= 1e3 && gumbel_scale >= 0.0 && gumbel_scale <= 8.0;
}

// a prior that has a logarithm: normal and finite (a NaN fails)
GZ_HD bool gumbel_prior_ok(double p) { return p >= GZ_GUMBEL_DBL_MIN && p <= GZ_GUMBEL_DBL_MAX; }

// any_ok: some empty cell of the row is ok (else every empty cell counts, with logit 0.0)
GZ_HD double gumbel_logit(double prior, bool any_ok) { return any_ok ? gz_log(prior) : 0.0; }

// g(c) of cell c
GZ_HD double gumbel_noise(uint64_t key, int c, double gumbel_scale) {
    const double u = unit_open(draw(key, (uint32_t)c));
    double e = -gz_log(u);
    if (!(e >= GZ_GUMBEL_DBL_MIN)) e = 0x1p-53;  // (u == 1)
    return gumbel_scale * (-gz_log(e));
}

// sigma(q) with the largest root-child visit count maxN
GZ_HD double gumbel_sigma(double c_visit, double c_scale, int maxN, double q) {
    return ((c_visit + (double)maxN) * c_scale) * q;
}

// the score of a considered cell at root selection (want: the schedule's count, n = want visits
// of its child) and at the move choice (want = n = the most visits)
GZ_HD double gumbel_score(double gs, double c_visit, double c_scale, int maxN, int want, double W, int n) {
    if (want == 0) return gs;
    return gs + gumbel_sigma(c_visit, c_scale, maxN, W / (double)n);
}

// seq(m, S) into out[S]: every considered child of a phase has the same count v, so a phase
// of x passes over k children is x runs of k equal entries
GZ_HD void gumbel_sequence(int m, int S, int16_t* out) {
    if (m <= 1) {
        for (int t = 0; t < S; t++) out[t] = (int16_t)t;
        return;
    }
    int L = 0;
    while ((1 << L) < m) L++;
    int k = m, v = 0, len = 0;
    while (len < S) {
        int x = S / (L * k);
        if (x < 1) x = 1;
        for (int r = 0; r < x && len < S; r++) {
            for (int i = 0; i < k && len < S; i++) out[len++] = (int16_t)v;
            v++;
        }
        k = k / 2 < 2 ? 2 : k / 2;
    }
}

// Root preparation of one row on the host: empty[c] non-zero = empty cell; gs[225] out.
// Returns m.  The device (gumbel_root, gz_puct.hip) runs the functions above with the
// arg-max across its lanes.
GZ_HD int gumbel_root_row(uint64_t key, const double* prior, const uint8_t* empty, int max_considered,
                          double gumbel_scale, double* gs) {
    bool any_ok = false;
    for (int c = 0; c < GZ_CELLS; c++)
        if (empty[c] && gumbel_prior_ok(prior[c])) any_ok = true;
    bool ok[GZ_CELLS];
    double base[GZ_CELLS];
    int n_ok = 0;
    for (int c = 0; c < GZ_CELLS; c++) {
        ok[c] = empty[c] && (!any_ok || gumbel_prior_ok(prior[c]));
        base[c] = 0.0;
        gs[c] = -__builtin_inf();
        if (!ok[c]) continue;
        n_ok++;
        base[c] = gumbel_noise(key, c, gumbel_scale) + gumbel_logit(prior[c], any_ok);
    }
    const int m = max_considered < n_ok ? max_considered : n_ok;
    for (int r = 0; r < m; r++) {
        int bc = -1;
        for (int c = 0; c < GZ_CELLS; c++)
            if (ok[c] && (bc < 0 || base[c] > base[bc])) bc = c;
        ok[bc] = false;
        gs[bc] = base[bc];
    }
    return m;
}

// (int32)(pi * 32767.0 + 0.5)
GZ_HD int32_t gumbel_row_entry(double pi) { return (int32_t)(pi * GZ_GUMBEL_ROW_SCALE + 0.5); }

// v_mix from the sums over the visited children
GZ_HD double gumbel_vmix(double v0, int sumN, double P, double A) {
    return (sumN > 0 && P > 0.0) ? (v0 + (double)sumN * (A / P)) / (1.0 + (double)sumN) : v0;
}

// The policy target of one row on the host: visits[c] == 0 means no child at c (W[c] is then
// not read).  empty == nullptr: every cell counts as empty, so the caller passes a prior that
// is not ok (0.0) at stones.  pi[225] and row[225] out (either may be nullptr).
GZ_HD void gumbel_policy_row(const double* prior, const uint8_t* empty, const double* W, const int32_t* visits,
                             double v0, double c_visit, double c_scale, double* pi, int32_t* row) {
    bool any_ok = false;
    for (int c = 0; c < GZ_CELLS; c++)
        if ((!empty || empty[c]) && gumbel_prior_ok(prior[c])) any_ok = true;
    int sumN = 0, maxN = 0;
    double P = 0.0, A = 0.0;
    for (int c = 0; c < GZ_CELLS; c++) {
        const int n = visits[c];
        if (n < 1) continue;
        sumN += n;
        if (n > maxN) maxN = n;
        P += prior[c];
        A += prior[c] * (W[c] / (double)n);
    }
    const double v_mix = gumbel_vmix(v0, sumN, P, A);
    double x[GZ_CELLS];
    bool ok[GZ_CELLS];
    double mx = 0.0;
    bool first = true;
    for (int c = 0; c < GZ_CELLS; c++) {
        ok[c] = (!empty || empty[c]) && (!any_ok || gumbel_prior_ok(prior[c]));
        x[c] = 0.0;
        if (!ok[c]) continue;
        const double cq = visits[c] >= 1 ? W[c] / (double)visits[c] : v_mix;
        x[c] = gumbel_logit(prior[c], any_ok) + gumbel_sigma(c_visit, c_scale, maxN, cq);
        if (first || x[c] > mx) mx = x[c];
        first = false;
    }
    double Z = 0.0;
    for (int c = 0; c < GZ_CELLS; c++) {
        if (!ok[c]) continue;
        x[c] = gz_exp(x[c] - mx);
        Z += x[c];
    }
    for (int c = 0; c < GZ_CELLS; c++) {
        const double p = ok[c] ? x[c] / Z : 0.0;
        if (pi) pi[c] = p;
        if (row) row[c] = ok[c] ? gumbel_row_entry(p) : 0;
    }
}

}  // namespace gz
