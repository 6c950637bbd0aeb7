// noise_hostcheck.cpp -- the root-noise sampler of csrc/gz_dirichlet.h on the host, as a
// stand-alone program for a sanitizer build (make -C tools noise_hostcheck):
//
//   g++ -std=c++17 -O1 -g -ffp-contract=off -fsanitize=address,undefined ...
//
// It runs the GZ_HD code the search runs (noise_gamma, noise_eta_row, noise_mix, gz_log,
// gz_exp) over the boards and parameters of the tests and checks what holds without a
// reference: eta is 0 at stones, non-negative and sums to 1, a board with one empty cell
// gives exactly 1.0 there, a full board gives the zero row, the mix of a distribution
// is a distribution, and log / exp stay within 4 ulp of libm.  Exit status 0: all held.
#include <cmath>
#include <cstdio>
#include <vector>

#include "../alphazero-gomoku_amd/csrc/gz_dirichlet.h"

using namespace gz;

static int fails = 0;

static void expect(bool ok, const char* what, double a, double b) {
    if (!ok) {
        std::printf("FAIL %s (%.17g, %.17g)\n", what, a, b);
        fails++;
    }
}

int main() {
    const double alphas[] = {1e-3, 0.03, 0.3, 1.0, 2.5, 1e3};
    const int64_t gids[] = {0, ((int64_t)1 << 40) + 3};
    const int plies[] = {0, 7, 199};
    std::vector<uint8_t> empty(GZ_CELLS), mid(GZ_CELLS), one(GZ_CELLS, 0), full(GZ_CELLS, 0);
    for (int c = 0; c < GZ_CELLS; c++) {
        empty[c] = 1;
        mid[c] = (c * 37 + 11) % 225 % 13 >= 5;
    }
    one[100] = 1;
    std::vector<double> eta(GZ_CELLS), prior(GZ_CELLS);
    int rows = 0;
    for (double alpha : alphas)
        for (int64_t gid : gids)
            for (int ply : plies) {
                const uint64_t key = stream_key(7, gid, ply, GZ_NOISE_SIM);
                for (const std::vector<uint8_t>* e : {&empty, &mid}) {
                    const bool ok = noise_eta_row(key, e->data(), alpha, eta.data());
                    double sum = 0.0, psum = 0.0, msum = 0.0;
                    int ne = 0;
                    for (int c = 0; c < GZ_CELLS; c++) ne += (*e)[c] != 0;
                    for (int c = 0; c < GZ_CELLS; c++) {
                        expect(eta[c] >= 0.0 && ((*e)[c] || eta[c] == 0.0), "eta at a cell", eta[c], c);
                        sum += eta[c];
                        prior[c] = (*e)[c] ? 1.0 / ne : 0.0;
                        psum += prior[c];
                        msum += (*e)[c] ? noise_mix(prior[c], 0.25, eta[c]) : prior[c];
                    }
                    expect(ok && std::fabs(sum - 1.0) < 1e-12, "eta sums to 1", sum, alpha);
                    expect(std::fabs(msum - psum) < 1e-12, "the mixed row sums to the prior's sum", msum, psum);
                    rows++;
                }
                // (at alpha 1e-3 the boost U^1000 underflows for half the draws: total 0, the zero row)
                const bool ok1 = noise_eta_row(key, one.data(), alpha, eta.data());
                expect(ok1 ? eta[100] == 1.0 : (alpha < 0.03 && eta[100] == 0.0), "one empty cell", eta[100], alpha);
                expect(!noise_eta_row(key, full.data(), alpha, eta.data()) && eta[0] == 0.0, "a full board", eta[0],
                       alpha);
            }
    // log / exp against libm, on the draws of one stream
    const uint64_t key = stream_key(1, 2, 3, GZ_NOISE_SIM);
    double worst_log = 0.0, worst_exp = 0.0;
    for (uint32_t i = 0; i < 200000; i++) {
        const double m = 0.5 + 0.5 * unit_open(draw(key, 2 * i));
        const double x = std::ldexp(m, (int)(draw(key, 2 * i + 1) % 64) - 60);
        const double want = std::log(x);
        if (want != 0.0) worst_log = std::fmax(worst_log, std::fabs(gz_log(x) - want) / std::fabs(want));
        const double y = -700.0 * unit_open(draw(key, 2 * i + 1));
        worst_exp = std::fmax(worst_exp, std::fabs(gz_exp(y) - std::exp(y)) / std::exp(y));
    }
    expect(worst_log <= 8.9e-16, "gz_log within 4 ulp", worst_log, 0);
    expect(worst_exp <= 8.9e-16, "gz_exp within 4 ulp", worst_exp, 0);
    expect(gz_exp(-708.5) == 0.0 && gz_exp(0.0) == 1.0 && gz_log(1.0) == 0.0, "edge arguments", gz_exp(-708.5), 0);
    std::printf("noise_hostcheck: %d rows, largest relative error gz_log %.3g gz_exp %.3g, %d failures\n", rows,
                worst_log, worst_exp, fails);
    return fails ? 1 : 0;
}
