// gz_pvsym.hip -- the policy-value forward under a board symmetry (gz_sym.h): the two
// kernels that sit on either side of gz_pv_forward, and the entry points built on them.
//
//   pv_sym_boards_kernel  one workgroup of 256 threads per row.  Thread b owns output bit
//                         b = 16 r + c: it reads its source cell's two bits from the row as
//                         staged in LDS (so out may be in: every read precedes every store),
//                         and a ballot per wave and colour assembles the two words of board
//                         rows 4 w .. 4 w + 3.  Guard positions (c = 15, r = 15) vote 0.  The
//                         row's t (given, or sym_of) is stored for the way back.
//   pv_sym_rows_kernel    one workgroup per 225-wide row, in place: the row is staged in
//                         LDS (coalesced loads), then cell c is stored from o_y[sym_dst(t, c)]
//                         (coalesced stores).  f32 logits, f32 probs and the f64 prior, each
//                         optional; the search paths pass the prior only.  Rows with t = 0
//                         and rows at or past min(*d_count, n) are left as they are.
//
// Neither kernel does arithmetic on the values: the mapped-back row is the forward's row of
// the transformed board, permuted, bit for bit.
#include <hip/hip_runtime.h>

#include "gz_internal.h"
#include "gz_sym.h"

using namespace gz;

namespace {

constexpr size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

__device__ inline int rows_valid(int n, const int32_t* d_count) {
    if (!d_count) return n;
    const int c = *d_count;
    return c < n ? c : n;
}

__global__ __launch_bounds__(256) void pv_sym_kernel(const uint32_t* boards, int n, uint64_t seed, uint8_t* sym) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    sym[i] = (uint8_t)sym_of(seed, boards + (size_t)i * 16);
}

__global__ __launch_bounds__(256) void pv_sym_boards_kernel(const uint32_t* in, uint32_t* out, int n,
                                                            const int32_t* d_count, const uint8_t* sym_in,
                                                            uint64_t seed, uint8_t* sym_out) {
    __shared__ uint32_t row[16];
    const int g = blockIdx.x;
    if (g >= rows_valid(n, d_count)) return;
    const int b = threadIdx.x;
    if (b < 16) row[b] = in[(size_t)g * 16 + b];
    __syncthreads();
    const int t = sym_in ? (sym_in[g] & 7) : sym_of(seed, row);
    const int r = b >> 4, c = b & 15;
    bool black = false, white = false;
    if (r < GZ_N && c < GZ_N) {
        const int s = cell_to_bit(sym_src(t, r * GZ_N + c));
        black = (row[s >> 5] >> (s & 31)) & 1u;
        white = (row[8 + (s >> 5)] >> (s & 31)) & 1u;
    }
    const uint64_t mb = __ballot(black), mw = __ballot(white);
    if ((b & 63) == 0) {
        const int w = b >> 6;  // the wave: words 2 w and 2 w + 1 of each colour
        uint2* o = (uint2*)(out + (size_t)g * 16);
        o[w] = make_uint2((uint32_t)mb, (uint32_t)(mb >> 32));
        o[4 + w] = make_uint2((uint32_t)mw, (uint32_t)(mw >> 32));
    }
    if (b == 0) sym_out[g] = (uint8_t)t;
}

__global__ __launch_bounds__(256) void pv_sym_rows_kernel(float* logits, float* probs, double* prior, int n,
                                                          const int32_t* d_count, const uint8_t* sym) {
    __shared__ float sl[GZ_CELLS];
    __shared__ float sp[GZ_CELLS];
    __shared__ double sd[GZ_CELLS];
    const int g = blockIdx.x;
    if (g >= rows_valid(n, d_count)) return;
    const int t = sym[g] & 7;
    if (t == 0) return;
    const int c = threadIdx.x;
    const size_t at = (size_t)g * GZ_CELLS + c;
    if (c < GZ_CELLS) {
        if (logits) sl[c] = logits[at];
        if (probs) sp[c] = probs[at];
        if (prior) sd[c] = prior[at];
    }
    __syncthreads();
    if (c < GZ_CELLS) {
        const int d = sym_dst(t, c);
        if (logits) logits[at] = sl[d];
        if (probs) probs[at] = sp[d];
        if (prior) prior[at] = sd[d];
    }
}

}  // namespace

extern "C" {

int gz_internal_sym_boards(const uint32_t* d_in, uint32_t* d_out, int32_t n, const int32_t* d_count,
                           const uint8_t* d_sym_in, uint64_t seed, uint8_t* d_sym_out, void* stream) {
    if (n <= 0) return GZ_OK;
    pv_sym_boards_kernel<<<n, 256, 0, (hipStream_t)stream>>>(d_in, d_out, n, d_count, d_sym_in, seed, d_sym_out);
    return gz_check_launch("pv_sym_boards_kernel");
}

int gz_internal_sym_rows(float* d_logits, float* d_probs, double* d_prior, int32_t n, const int32_t* d_count,
                         const uint8_t* d_sym, void* stream) {
    if (n <= 0 || (!d_logits && !d_probs && !d_prior)) return GZ_OK;
    pv_sym_rows_kernel<<<n, 256, 0, (hipStream_t)stream>>>(d_logits, d_probs, d_prior, n, d_count, d_sym);
    return gz_check_launch("pv_sym_rows_kernel");
}

int gz_pv_sym(const uint32_t* d_boards, int32_t n, uint64_t seed, uint8_t* d_sym, void* stream) {
    if (n < 0 || (n > 0 && (!d_boards || !d_sym))) return gz_fail(GZ_ERR_ARG, "gz_pv_sym: bad arguments");
    if (n == 0) return GZ_OK;
    pv_sym_kernel<<<(n + 255) / 256, 256, 0, (hipStream_t)stream>>>(d_boards, n, seed, d_sym);
    return gz_check_launch("pv_sym_kernel");
}

int gz_pv_sym_host(uint64_t seed, const uint32_t row[16]) {
    if (!row) return gz_fail(GZ_ERR_ARG, "gz_pv_sym_host: row is NULL");
    return sym_of(seed, row);
}

size_t gz_pv_sym_workspace_bytes(int32_t n) {
    if (n < 1) n = 1;
    return al256(gz_pv_workspace_bytes(n)) + al256((size_t)n * 64) + al256((size_t)n);
}

int gz_pv_forward_sym(const float* d_weights, const uint32_t* d_boards, int32_t n, const int32_t* d_count,
                      const uint8_t* d_sym, uint64_t seed, float* d_logits, float* d_value, float* d_probs,
                      double* d_prior, void* d_workspace, int32_t precision, void* stream) {
    if (n < 0 || (n > 0 && (!d_weights || !d_boards || !d_logits || !d_value)))
        return gz_fail(GZ_ERR_ARG, "gz_pv_forward_sym: bad arguments");
    if (precision != GZ_PV_FP32 && precision != GZ_PV_F16X3 && precision != GZ_PV_F16)
        return gz_fail(GZ_ERR_ARG, "gz_pv_forward_sym: unknown precision");
    if (!d_workspace) return gz_fail(GZ_ERR_ARG, "gz_pv_forward_sym: d_workspace is required");
    if (d_prior && !d_probs)
        return gz_fail(GZ_ERR_ARG,
                       "gz_pv_forward_sym: d_prior needs d_probs (the prior is renormalised from the softmax)");
    if (n == 0) return GZ_OK;
    char* p = (char*)d_workspace + al256(gz_pv_workspace_bytes(n));
    uint32_t* y = (uint32_t*)p;
    uint8_t* t = (uint8_t*)(p + al256((size_t)n * 64));
    int rc = gz_internal_sym_boards(d_boards, y, n, d_count, d_sym, seed, t, stream);
    if (rc) return rc;
    rc = gz_pv_forward(d_weights, y, n, d_count, d_logits, d_value, d_probs, d_prior, d_workspace, precision, stream);
    if (rc) return rc;
    return gz_internal_sym_rows(d_logits, d_probs, d_prior, n, d_count, t, stream);
}

}  // extern "C"
