// gz_dirichlet.h -- the Dirichlet noise of the PUCT search root (opt-in,
// GZ_PUCT_ROOT_NOISE): prior' = (1 - eps) prior + eps eta, eta ~ Dir(alpha) over the
// empty cells.  tests/puct_noise_ref.py restates every line in Python, bit for bit.
//
// Stream: key = stream_key(seed, game id, the root's move count, GZ_NOISE_SIM); cell c
// (row-major) owns the draws 256 c + i, 0 <= i < 256, of that key, so a cell's sample
// does not depend on the lane (or host loop) that computes it.
//
// Everything is GZ_HD and uses only + - * /, frexp, ldexp, floor and sqrt on doubles,
// in the order written, so the device, the host and CPython round alike.  The unit
// that includes this header is compiled with -ffp-contract=off (no fused multiply-add).
#pragma once
#include "gz_bitboard.h"

namespace gz {

static constexpr int32_t GZ_NOISE_SIM = 0x4E4F4953;  // simulation streams use sim <= 4095
static constexpr int GZ_NOISE_DRAWS = 256;           // draws a cell owns

// ((x >> 11) + 1) 2^-53: in (0, 1], exact
GZ_HD double unit_open(uint64_t x) { return (double)((x >> 11) + 1) * (1.0 / 9007199254740992.0); }

// log(x), x > 0 finite and normal: x = m 2^e with m in [sqrt(1/2), sqrt(2)),
// log(m) = 2 atanh(s), s = (m - 1)/(m + 1), the series to s^23 by Horner
GZ_HD double gz_log(double x) {
    const double LN2_HI = 0x1.62e42fee00000p-1, LN2_LO = 0x1.a39ef35793c76p-33;
    const double SQRT_HALF = 0x1.6a09e667f3bcdp-1;
    int e;
    double m = __builtin_frexp(x, &e);
    if (m < SQRT_HALF) {
        m = m * 2.0;
        e -= 1;
    }
    const double s = (m - 1.0) / (m + 1.0);
    const double z = s * s;
    double p = 1.0 / 23.0;
    p = p * z + 1.0 / 21.0;
    p = p * z + 1.0 / 19.0;
    p = p * z + 1.0 / 17.0;
    p = p * z + 1.0 / 15.0;
    p = p * z + 1.0 / 13.0;
    p = p * z + 1.0 / 11.0;
    p = p * z + 1.0 / 9.0;
    p = p * z + 1.0 / 7.0;
    p = p * z + 1.0 / 5.0;
    p = p * z + 1.0 / 3.0;
    p = p * z + 1.0 / 1.0;
    const double de = (double)e;
    return (de * LN2_HI + (2.0 * s) * p) + de * LN2_LO;
}

// exp(x), x <= 0 (0 below -708, so the result stays normal): x = k ln2 + r,
// |r| <= ln2 / 2, the Taylor series to r^13 by Horner
GZ_HD double gz_exp(double x) {
    const double LN2_HI = 0x1.62e42fee00000p-1, LN2_LO = 0x1.a39ef35793c76p-33;
    const double INV_LN2 = 0x1.71547652b82fep+0;
    if (x < -708.0) return 0.0;
    const double k = __builtin_floor(x * INV_LN2 + 0.5);
    const double r = (x - k * LN2_HI) - k * LN2_LO;
    double p = 1.0 / 6227020800.0;
    p = p * r + 1.0 / 479001600.0;
    p = p * r + 1.0 / 39916800.0;
    p = p * r + 1.0 / 3628800.0;
    p = p * r + 1.0 / 362880.0;
    p = p * r + 1.0 / 40320.0;
    p = p * r + 1.0 / 5040.0;
    p = p * r + 1.0 / 720.0;
    p = p * r + 1.0 / 120.0;
    p = p * r + 1.0 / 24.0;
    p = p * r + 1.0 / 6.0;
    p = p * r + 1.0 / 2.0;
    p = p * r + 1.0 / 1.0;
    p = p * r + 1.0 / 1.0;
    return __builtin_ldexp(p, (int)k);
}

// Gamma(alpha, 1) for cell c: Marsaglia-Tsang on alpha + 1 with polar normals, boosted
// by U^(1/alpha); 0.0 when the cell's draws run out (never seen: 28 of 256 at most)
GZ_HD double noise_gamma(uint64_t key, int c, double alpha) {
    const uint32_t base = (uint32_t)(GZ_NOISE_DRAWS * c);
    const double d = (alpha + 1.0) - 1.0 / 3.0;
    const double cc = 1.0 / __builtin_sqrt(9.0 * d);
    double v = 0.0;
    int i = 1;
    while (true) {
        if (i + 3 > GZ_NOISE_DRAWS) return 0.0;
        const double a = 2.0 * unit_open(draw(key, base + i)) - 1.0;
        const double b = 2.0 * unit_open(draw(key, base + i + 1)) - 1.0;
        const double u = unit_open(draw(key, base + i + 2));
        i += 3;
        const double s = a * a + b * b;
        if (s >= 1.0 || s == 0.0) continue;
        const double x = a * __builtin_sqrt((-2.0 * gz_log(s)) / s);
        const double t = 1.0 + cc * x;
        if (t <= 0.0) continue;
        v = (t * t) * t;
        if (gz_log(u) < (((0.5 * x) * x + d) - d * v) + d * gz_log(v)) break;
    }
    return (d * v) * gz_exp(gz_log(unit_open(draw(key, base))) / alpha);
}

GZ_HD bool noise_total_ok(double total) { return total > 0.0 && total <= 1.7976931348623157e308; }

GZ_HD double noise_mix(double prior, double eps, double eta) { return (1.0 - eps) * prior + eps * eta; }

// The sequential form (the host entry point): eta[225] from empty[225] (non-zero =
// empty cell); total is one running sum over the empty cells in ascending order.
// All zero, and false, when total is 0 or not finite.
GZ_HD bool noise_eta_row(uint64_t key, const uint8_t* empty, double alpha, double* eta) {
    double total = 0.0;
    for (int c = 0; c < GZ_CELLS; c++) {
        eta[c] = empty[c] ? noise_gamma(key, c, alpha) : 0.0;
        if (empty[c]) total += eta[c];
    }
    const bool ok = noise_total_ok(total);
    for (int c = 0; c < GZ_CELLS; c++) eta[c] = (ok && empty[c]) ? eta[c] / total : 0.0;
    return ok;
}

}  // namespace gz
