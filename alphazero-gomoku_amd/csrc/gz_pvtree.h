// gz_pvtree.h -- device pieces the two incremental tree kernels share: pv_sib_kernel
// (gz_pvinc.hip, grandchildren: exact windows) and pv_dg_kernel (gz_pvdg.hip, root
// children: D squares).  Only what both can take without a change to their code; their
// k-loops, fills, epilogues and conv0 bodies differ on purpose and stay in their files.
// (The conv0 im2col and the record overlay's index classification are the same
// computation in both too, but either kernel's instruction stream changes with the
// spelling of the other's, so each file keeps its own.)
#pragma once
#include <hip/hip_runtime.h>

#include "gz_f16conv.h"
#include "gz_pvnet.h"

namespace gzpv {

// A node's patch: the recomputed squares of its maps (x0 r1, y1 r2, x1 r3, y2 r4),
// [plane][16 cg][(2r+1)^2][8] each, in that order -- also the layout of a node's squares
// in pv_sib_kernel's scratch
constexpr int PATCH_OFF[4] = {0, 9 * 256, 34 * 256, 83 * 256};  // halves
constexpr int PATCH_HALVES = PV_PATCH_HALVES;

__device__ inline int iabs(int x) { return x < 0 ? -x : x; }

// LDS-DMA (global_load_lds) operands, and the 16 zero bytes its fills read for
// positions off the board or past the nodes' squares
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) void glb_void_t;
static __device__ uint4 gz_tree_zero16[1];  // zero-initialised

// the square of radius rl around (cr, cc), clipped to the board, row-major
struct Rows {
    int r0, c0, wr, n;
};
__device__ inline Rows make_rows(int cr, int cc, int rl) {
    Rows q;
    q.r0 = cr - rl < 0 ? 0 : cr - rl;
    const int r1 = cr + rl > gzc::BN - 1 ? gzc::BN - 1 : cr + rl;
    q.c0 = cc - rl < 0 ? 0 : cc - rl;
    const int c1 = cc + rl > gzc::BN - 1 ? gzc::BN - 1 : cc + rl;
    q.wr = c1 - q.c0 + 1;
    q.n = (r1 - q.r0 + 1) * q.wr;
    return q;
}

// Phase stamps (tools/pvinc_bench.py only): a stamp build (ACC = the kernel's tick
// array) accumulates s_memtime deltas of workgroup 0 / thread 0 per phase (vector
// atomics); otherwise (ACC = nullptr) compiled out.
template <unsigned long long* ACC>
struct PhaseStamp {
    unsigned long long t = __builtin_amdgcn_s_memtime();
    __device__ void operator()(int i) {
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            const unsigned long long t_ = __builtin_amdgcn_s_memtime();
            atomicAdd(&ACC[i], t_ - t);
            t = t_;
        }
    }
};
template <>
struct PhaseStamp<nullptr> {
    __device__ void operator()(int) {}
};

}  // namespace gzpv
