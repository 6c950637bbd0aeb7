// gz_pvtree.h -- device pieces of the incremental tree kernel pv_dg_kernel (gz_pvdg.hip:
// root children as a delta of their root, grandchildren as a delta of their parent).
#pragma once
#include <hip/hip_runtime.h>

#include "gz_f16conv.h"
#include "gz_pvnet.h"

namespace gzpv {

// A parent's patch (gz_pvnet.h): fp32 [position][128]; the first position of its x0 r1
// (post-ReLU), then of its pre-ReLU y1 r2, x1 r3, y2 r4, x2 r5 squares, each row-major
// around its stone (unclipped index; off-board positions unwritten)
constexpr int PATCH_POS[5] = {0, 9, 34, 83, 164};
constexpr int PATCH_FLOATS = PV_PATCH_POS * CH;
static_assert(PATCH_POS[4] + 121 == PV_PATCH_POS, "patch positions");

__device__ inline int iabs(int x) { return x < 0 ? -x : x; }

// LDS-DMA (global_load_lds) operands, and the 16 zero bytes its fills read for
// positions off the board or past the nodes' squares
typedef __attribute__((address_space(3))) void lds_void_t;
typedef __attribute__((address_space(1))) void glb_void_t;
static __device__ uint4 gz_tree_zero16[1];  // zero-initialised

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
