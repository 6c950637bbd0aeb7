// gz_pvinc.hip -- the classification kernels of the incremental policy-value forward
// (gz_pv_forward_tree; AlphaZeroGomokuNet, neural_network.py:74-159, f16x3 precision).
//
// MCTSNode.__init__ runs GomokuModel.predict for every new node (ai_agent.py:
// 522-523).  A root child differs from the root by one stone at cell m, so in
// layer L of the tower (x0 = conv0, y1, x1, y2, x2) only the positions within
// Chebyshev radius L+1 of m can differ from the root's maps: 3x3, 5x5, 7x7, 9x9,
// 11x11 squares (clipped to the board) -- about 31 % of the 4 x 225 positions of
// the residual convs.  The root is evaluated by the full kernel, which also stores
// its x0, y1, x1, y2 maps and its pre-ReLU values (gz_pvnet.hip,
// pv_kernel_f16x3<.., true>).  The root children are computed as a delta of the
// root's by pv_dg_kernel (gz_pvdg.hip); a child with children of its own also stores
// its pre-ReLU values in its changed squares (its "patch"), and its children (the
// grandchildren, one more stone at m2) are computed by the same kernel as a delta of
// THEIR parent: the parent's patch inside its squares, the root's values elsewhere.
//
// Here: which leaf is a root, a root child, a grandchild or none of them (the full
// forward), the lists the kernels work through, and the patch slots.
#include <hip/hip_runtime.h>

#include "gz_internal.h"
#include "gz_pvtree.h"

using namespace gzpv;

namespace {

using namespace gzc;

// one thread per leaf: roots (meta -1) take the next map slot (ord), others -1;
// no patch slot yet
__global__ void tree_roots_kernel(const int32_t* __restrict__ meta, int n, const int32_t* __restrict__ d_count,
                                  int root_cap, int32_t* __restrict__ ord, int32_t* __restrict__ pslot,
                                  int32_t* __restrict__ ctr) {
    const int count = d_count ? (*d_count < n ? *d_count : n) : n;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    int o = -1;
    if (meta[i] == -1) {
        o = atomicAdd(&ctr[CTR_ROOTS_SEEN], 1);
        if (o >= root_cap) o = -1;
    }
    ord[i] = o;
    pslot[i] = -1;
}

// node classes (ord: roots' map slots): a root child = meta m >= 0 with ord[m] >= 0;
// a grandchild = meta m >= 0 whose m is such a root child
// boards i and j differ in exactly one bit (one cell changed).  The tags are the
// caller's claim; a leaf whose board does not differ from its tagged parent by one
// cell simply takes the full forward, so a wrong tag costs time, never results
__device__ inline bool one_cell(const uint32_t* __restrict__ boards, int i, int j) {
    int bits = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) bits += __popc(boards[(size_t)i * 16 + k] ^ boards[(size_t)j * 16 + k]);
    return bits == 1;
}

// leaf i is a child of the mapped root m
__device__ inline bool is_child(const int32_t* ord, const uint32_t* boards, int i, int m, int count) {
    return m >= 0 && m < count && ord[m] >= 0 && one_cell(boards, i, m);
}

// one thread per grandchild: its parent claims a patch slot (first come; -2 while
// being claimed, -3 once the slots are exhausted)
__global__ void tree_patch_kernel(const int32_t* __restrict__ meta, int n, const int32_t* __restrict__ d_count,
                                  const int32_t* __restrict__ ord, const uint32_t* __restrict__ boards, int patch_cap,
                                  int32_t* __restrict__ pslot, int32_t* __restrict__ ctr) {
    const int count = d_count ? (*d_count < n ? *d_count : n) : n;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int m = meta[i];
    if (m < 0 || m >= count || !is_child(ord, boards, m, meta[m], count) || !one_cell(boards, i, m)) return;
    if (atomicCAS(&pslot[m], -1, -2) == -1) {
        const int s = atomicAdd(&ctr[CTR_PATCHES], 1);
        pslot[m] = s < patch_cap ? s : -3;
    }
}

// lists: roots with a map slot (full forward + maps), every board that is neither
// a root child nor a grandchild whose parent has a patch (full forward); one atomic
// per wave and list.  Grandchildren are chained per parent (ghead / gnext) for
// tree_grand_order_kernel
__device__ inline void wave_append(bool take, int i, int32_t* ctr, int32_t* list) {
    const uint64_t m = __ballot(take);
    if (!m) return;
    int base = 0;
    const int lane = threadIdx.x & 63;
    const int leader = __ffsll((unsigned long long)m) - 1;
    if (lane == leader) base = atomicAdd(ctr, __popcll(m));
    base = __shfl(base, leader);
    if (take) list[base + __popcll(m & ((1ull << lane) - 1))] = i;
}

// the cell of the one stone where boards a and b (16-word leaf rows) differ
__device__ inline int stone_cell(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b) {
    int cell = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const uint32_t d = a[k] ^ b[k];
        if (d) {
            const int bit = (k & 7) * 32 + __builtin_ctz(d);
            cell = (bit >> 4) * BN + (bit & 15);
        }
    }
    return cell;
}

__global__ void tree_lists_kernel(const int32_t* __restrict__ meta, int n, const int32_t* __restrict__ d_count,
                                  const int32_t* __restrict__ ord, const int32_t* __restrict__ pslot,
                                  const uint32_t* __restrict__ boards, int32_t* __restrict__ ctr,
                                  int32_t* __restrict__ roots, int32_t* __restrict__ full, int32_t* __restrict__ ghead,
                                  int32_t* __restrict__ gnext, int32_t* __restrict__ cinfo,
                                  int32_t* __restrict__ wcount) {
    const int count = d_count ? (*d_count < n ? *d_count : n) : n;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const bool valid = i < count;
    const int m = valid ? meta[i] : -3;
    const bool root = valid && m == -1 && ord[i] >= 0;
    const bool child = valid && is_child(ord, boards, i, m, count);
    const bool gc = valid && !child && m >= 0 && m < count && pslot[m] >= 0 && is_child(ord, boards, m, meta[m], count) &&
                    one_cell(boards, i, m);
    wave_append(root, i, ctr + CTR_ROOTS, roots);
    wave_append(valid && !root && !child && !gc, i, ctr + CTR_FULL, full);
    if (gc) gnext[i] = atomicExch(&ghead[pslot[m]], i);  // per parent, any order
    if (valid) {  // the incremental kernels' per-leaf word: root map slot and stone cell
        int ci = -1;
        if (child || gc) {
            const int o = ord[child ? m : meta[m]];
            ci = (gc ? 1 << 30 : 0) | (o << 8) | stone_cell(boards + (size_t)i * 16, boards + (size_t)m * 16);
        }
        cinfo[i] = ci;
    }
    // root children: counted here, listed in leaf order by tree_children_kernel
    const uint64_t c = __ballot(child);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(ctr + CTR_CHILDREN, __popcll(c));
    if ((threadIdx.x & 63) == 0 && i < n) wcount[i >> 6] = __popcll(c);  // lane 0: i = 64 w
}

// pv_dg_kernel's work list: the root children in LEAF order (a root's children are
// adjacent leaves, so neighbouring list entries share a root's maps).  wcount[w] =
// root children among leaves [64 w, 64 w + 64) (tree_lists_kernel); one workgroup
// of 1024 threads scans the counts in tiles, then (tree_children_scatter_kernel) each
// group's wave writes its leaves' list entries.  cinfo >= 0 with bit 30 clear marks a
// root child.
__global__ __launch_bounds__(1024) void tree_children_kernel(int n, const int32_t* __restrict__ d_count,
                                                            const int32_t* __restrict__ cinfo,
                                                            int32_t* __restrict__ wcount,
                                                            int32_t* __restrict__ children) {
    __shared__ int wsum[16];
    __shared__ int carry;
    const int count = d_count ? (*d_count < n ? *d_count : n) : n;
    const int nw = (count + 63) >> 6;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) carry = 0;
    __syncthreads();
    // exclusive scan of wcount in place, 1024 entries per tile
    for (int t0 = 0; t0 < nw; t0 += 1024) {
        const int w = t0 + tid;
        const int v = w < nw ? wcount[w] : 0;
        int x = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int y = __shfl_up(x, d);
            if (lane >= d) x += y;
        }
        if (lane == 63) wsum[wv] = x;
        __syncthreads();
        if (tid < 16) {
            int y = wsum[tid];
            for (int d = 1; d < 16; d <<= 1) {
                const int z = __shfl_up(y, d, 16);
                if (tid >= d) y += z;
            }
            wsum[tid] = y;  // inclusive over waves
        }
        __syncthreads();
        const int base = carry + (wv ? wsum[wv - 1] : 0);
        if (w < nw) wcount[w] = base + x - v;
        __syncthreads();
        if (tid == 0) carry += wsum[15];
        __syncthreads();
    }
}

// then one wave per 64-leaf group (the loop of 16 waves over the groups was a chain of
// dependent load latencies, 0.4 ms per forward): the group's children in lane order at its
// scanned offset
__global__ __launch_bounds__(1024) void tree_children_scatter_kernel(int n, const int32_t* __restrict__ d_count,
                                                                    const int32_t* __restrict__ cinfo,
                                                                    const int32_t* __restrict__ wcount,
                                                                    int32_t* __restrict__ children) {
    const int count = d_count ? (*d_count < n ? *d_count : n) : n;
    const int w = blockIdx.x * 16 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (w * 64 >= count) return;
    const int i = w * 64 + lane;
    const int ci = i < count ? cinfo[i] : -1;
    const bool child = ci >= 0 && !(ci & (1 << 30));
    const uint64_t m = __ballot(child);
    if (child) children[wcount[w] + __popcll(m & ((1ull << lane) - 1))] = i;
}

// the grandchild list in PARENT order: one thread per leaf; a parent with a patch
// appends its grandchildren (its ghead / gnext chain), a wave's parents in lane
// order.  A root's children are adjacent leaves, so a root's grandchildren end up
// adjacent in the list (the search reserves them one by one during its sequential
// phase, interleaved with every other game's), and pv_dg_kernel's XCD-contiguous
// eighths of the list then keep each root's maps in one L2
__global__ void tree_grand_order_kernel(int n, const int32_t* __restrict__ d_count, const int32_t* __restrict__ pslot,
                                        const int32_t* __restrict__ ghead, const int32_t* __restrict__ gnext,
                                        int32_t* __restrict__ ctr, int32_t* __restrict__ grand) {
    const int count = d_count ? (*d_count < n ? *d_count : n) : n;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int ps = i < count ? pslot[i] : -1;
    const int h = ps >= 0 ? ghead[ps] : -1;
    int k = 0;
    for (int g = h; g >= 0; g = gnext[g]) k++;
    // wave prefix sum of k, one atomic per wave
    const int lane = threadIdx.x & 63;
    int incl = k;
    for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d);
        if (lane >= d) incl += v;
    }
    const int total = __shfl(incl, 63);
    int base = 0;
    if (lane == 63 && total) base = atomicAdd(ctr + CTR_GRAND, total);
    base = __shfl(base, 63);
    int at = base + incl - k;
    for (int g = h; g >= 0; g = gnext[g]) grand[at++] = g;
}

}  // namespace

// Launches of the incremental forward's own kernels (called by gz_pv_forward_tree in
// gz_pvnet.hip, which runs the full kernel on the root and full lists in between).
int gz_internal_tree_classify(const TreeWs& t, const uint32_t* d_boards, const int32_t* d_meta, int32_t n,
                              const int32_t* d_count, int32_t root_cap, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (hipMemsetAsync(t.ctr, 0, CTR_COUNT * sizeof(int32_t), s) != hipSuccess ||  // (the queue heads too)
        (t.patch_cap > 0 && hipMemsetAsync(t.ghead, 0xff, (size_t)t.patch_cap * sizeof(int32_t), s) != hipSuccess))
        return gz_fail(GZ_ERR_HIP, "gz_pv_forward_tree: memset");
    const int g = (n + 255) / 256;
    tree_roots_kernel<<<g, 256, 0, s>>>(d_meta, n, d_count, root_cap, t.ord, t.pslot, t.ctr);
    tree_patch_kernel<<<g, 256, 0, s>>>(d_meta, n, d_count, t.ord, d_boards, t.patch_cap, t.pslot, t.ctr);
    // per-wave child counts: past the list's n entries (t.children has n + n / 64 + 1)
    int32_t* wcount = t.children + n;
    tree_lists_kernel<<<g, 256, 0, s>>>(d_meta, n, d_count, t.ord, t.pslot, d_boards, t.ctr, t.roots, t.full, t.ghead,
                                        t.gnext, t.cinfo, wcount);
    tree_children_kernel<<<1, 1024, 0, s>>>(n, d_count, t.cinfo, wcount, t.children);
    tree_children_scatter_kernel<<<(n + 1023) / 1024, 1024, 0, s>>>(n, d_count, t.cinfo, wcount, t.children);
    tree_grand_order_kernel<<<g, 256, 0, s>>>(n, d_count, t.pslot, t.ghead, t.gnext, t.ctr, t.grand);
    return gz_check_launch("tree classify");
}

// the root children, then the grandchildren, through pv_dg_kernel (gz_pvdg.hip)
int gz_internal_tree_children(const TreeWs& t, const float* d_weights, const uint32_t* d_boards,
                              const int32_t* d_meta, int32_t n, const int32_t* d_count, int grid, void* stream) {
    return gz_internal_tree_delta(t, d_weights, d_boards, d_meta, grid, stream);
}
