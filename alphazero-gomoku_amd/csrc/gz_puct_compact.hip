// gz_puct_compact.hip -- slot compaction of a PUCT self-play engine
// (gz_selfplay_puct_compact; in place; tests/puct_compact_ref.py restates it).
//
// With a active slots among the first n_active, the holes are the idle slots below a and the
// fillers the active ones at or above a; there are equally many, and the k-th filler goes to
// the k-th hole (both ascending).  Sources (>= a) and destinations (< a) are disjoint, so all
// pairs move at once without a second copy of the trees or of pend; the slot order is not
// preserved.
//   1. puct_compact_plan_kernel   one workgroup: counts a, ranks holes and fillers, writes
//                                 the pair lists, d_order and d_n_active;
//   2. puct_compact_move_kernel   pair x part: the filler's pend rows [0, n_moves) and, for
//                                 the reuse engine, its PuctHdr and rows [0, n_nodes) of
//                                 each tree array to the hole's places, byte for byte
//                                 (16-byte words between the unaligned ends of a span);
//   3. puct_compact_swap_kernel   the two slot buffers trade places (after 2, which reads
//                                 n_moves from the filler's slot where it was).
// The launches are sized for the most pairs there can be, n_active / 2; a workgroup past
// the device's pair count leaves at once.  What a hole held, and a filler's old place, are
// dead: an idle slot is never searched, and a later filler overwrites all that is read.
// The layouts that are moved -- pend, the PuctHdr and the node record -- are gz_puct.h's.
#include "gz_puct.h"

using namespace gz;

namespace {

// The plan in the workspace: int32 n_pairs (16 bytes), holes [cap], fillers [cap].
constexpr int CP_THREADS = 256;
constexpr int CP_PARTS = 8;  // workgroups that share the bytes of one pair

// One workgroup scans the first n slots in tiles of 1024 (rank_two_classes): pass 0 counts
// the active slots, a; pass 1 ranks the holes (idle, index < a) and the fillers (active,
// index >= a), each ascending; then the k-th filler is paired with the k-th hole.
// order[s] = s except at the pairs, which trade places.
__global__ __launch_bounds__(1024) void puct_compact_plan_kernel(const char* slots, int n, int cap, int32_t* order,
                                                                 int32_t* n_active, int32_t* plan) {
    __shared__ int carry[2], total;
    const int tid = threadIdx.x;
    int32_t* holes = plan + 4;
    int32_t* fillers = holes + cap;
    for (int pass = 0; pass < 2; pass++) {
        if (tid == 0) carry[0] = carry[1] = 0;
        __syncthreads();
        for (int t0 = 0; t0 < n; t0 += 1024) {
            const int s = t0 + tid;
            const bool in = s < n;
            bool act = false;
            if (in) {
                const SlotHeader* h = slot_of(slots, s);
                act = h->game_id < h->game_id_end;
            }
            // (pass 0: x = active; pass 1: x = hole, y = filler)
            const bool x = pass == 0 ? act : (in && !act && s < total);
            const bool y = pass == 1 && act && s >= total;
            int rx, ry;
            rank_two_classes(x, y, carry, rx, ry);
            if (pass == 1) {
                if (x) holes[rx] = s;
                if (y) fillers[ry] = s;
                if (in && !x && !y) order[s] = s;
            }
        }
        if (tid == 0 && pass == 0) {
            total = carry[0];
            *n_active = carry[0];
        }
        __syncthreads();
    }
    // (as many fillers as holes: a minus the active slots below a, either way)
    const int pairs = carry[0] < carry[1] ? carry[0] : carry[1];
    if (tid == 0) plan[0] = pairs;
    __threadfence_block();  // the lists are written before other threads of the workgroup read them
    __syncthreads();
    for (int k = tid; k < pairs; k += 1024) {
        const int h = holes[k], f = fillers[k];
        order[h] = f;
        order[f] = h;
    }
}

// nbytes from src to dst, which are congruent mod 16: this workgroup's share (part of
// CP_PARTS) of the 16-byte words between the unaligned ends, and the ends by part 0
__device__ inline void copy_span(char* dst, const char* src, size_t nbytes, int part) {
    size_t head = (16 - ((size_t)src & 15)) & 15;
    if (head > nbytes) head = nbytes;
    const size_t words = (nbytes - head) / 16;
    const uint4* a = (const uint4*)(src + head);
    uint4* b = (uint4*)(dst + head);
    for (size_t i = (size_t)part * CP_THREADS + threadIdx.x; i < words; i += (size_t)CP_PARTS * CP_THREADS) b[i] = a[i];
    if (part == 0 && threadIdx.x < 16) {
        const size_t t = head + words * 16 + threadIdx.x;
        if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
        if (t < nbytes) dst[t] = src[t];
    }
}

// Pair k (blockIdx.x), part blockIdx.y: the filler's pending visit rows [0, n_moves) and,
// with trees, its tree (the header and rows [0, n_nodes) of every array) to the hole's
// places.  The slots are still where they were (puct_compact_swap_kernel runs afterwards).
__global__ __launch_bounds__(CP_THREADS) void puct_compact_move_kernel(const char* slots, const int32_t* plan, int cap,
                                                                       int S, int trees, char* ws, uint16_t* pend) {
    const int k = blockIdx.x, part = blockIdx.y;
    if (k >= plan[0]) return;
    const int h = plan[4 + k], f = plan[4 + cap + k];
    int rows = slot_of(slots, f)->n_moves;
    rows = rows < 0 ? 0 : (rows > GZ_MAX_GAME_PLIES ? GZ_MAX_GAME_PLIES : rows);
    const size_t per_slot = (size_t)GZ_MAX_GAME_PLIES * GZ_CELLS * 2;
    copy_span((char*)pend + h * per_slot, (const char*)pend + f * per_slot, (size_t)rows * GZ_CELLS * 2, part);
    if (!trees) return;
    const size_t M = (size_t)S + 1;
    const char* src = ws + 256 + f * game_stride_for(S);
    char* dst = ws + 256 + h * game_stride_for(S);
    int nn = ((const PuctHdr*)src)->n_nodes;
    nn = nn < 0 ? 0 : (nn > S + 1 ? S + 1 : nn);
    copy_span(dst, src, sizeof(PuctHdr), part);
    for (int a = 0; a < NODE_FIELDS; a++)  // rows [0, n_nodes) of every array, where tree_of finds them
        copy_span(dst + sizeof(PuctHdr) + node_offset(a) * M, src + sizeof(PuctHdr) + node_offset(a) * M,
                  node_width(a) * nn, part);
}

// the slot buffers of pair k trade places (16-byte words)
__global__ __launch_bounds__(CP_THREADS) void puct_compact_swap_kernel(char* slots, const int32_t* plan, int cap) {
    const int k = blockIdx.x, part = blockIdx.y;
    if (k >= plan[0]) return;
    const size_t sb = slot_stride_bytes();
    uint4* a = (uint4*)(slots + plan[4 + k] * sb);
    uint4* b = (uint4*)(slots + plan[4 + cap + k] * sb);
    for (size_t i = (size_t)part * CP_THREADS + threadIdx.x; i < sb / 16; i += (size_t)CP_PARTS * CP_THREADS) {
        const uint4 x = a[i], y = b[i];
        a[i] = y;
        b[i] = x;
    }
}

}  // namespace

extern "C" {

size_t gz_selfplay_puct_compact_workspace_bytes(int32_t n_slots) {
    return al256(16 + 2 * (size_t)(n_slots > 0 ? n_slots : 0) * 4);
}

int gz_selfplay_puct_compact(void* d_slots, int32_t n_slots, int32_t n_active, int32_t S, int32_t K,
                             int32_t move_trees, void* d_puct_workspace, int32_t* d_order, int32_t* d_n_active,
                             void* d_workspace, void* stream) {
    int rc = check_S("gz_selfplay_puct_compact", n_slots, S);
    if (rc) return rc;
    if (!d_slots || n_slots < 1 || !d_puct_workspace || !d_order || !d_n_active || !d_workspace)
        return gz_fail(GZ_ERR_ARG, "gz_selfplay_puct_compact: bad arguments");
    rc = check_active("gz_selfplay_puct_compact", n_active, n_slots);
    if (rc) return rc;
    if (K < 0 || K > GZ_PUCT_MAX_LEAVES)  // (0: the unbatched search, as PuctCfg.leaves)
        return gz_fail(GZ_ERR_ARG, "gz_selfplay_puct_compact: leaves_per_round out of range [0, 32]");
    if (K > 1 && move_trees)
        return gz_fail(GZ_ERR_ARG, "gz_selfplay_puct_compact: tree reuse with leaves_per_round > 1 is not supported");
    const SelfplayWs w = carve_selfplay(d_puct_workspace, n_slots);
    int32_t* plan = (int32_t*)d_workspace;
    hipStream_t st = as_stream(stream);
    puct_compact_plan_kernel<<<1, 1024, 0, st>>>((const char*)d_slots, n_active, n_slots, d_order, d_n_active, plan);
    rc = gz_check_launch("puct_compact_plan_kernel");
    if (rc) return rc;
    const int pairs = n_active / 2;  // at most: the count itself stays on the device
    if (pairs == 0) return GZ_OK;
    puct_compact_move_kernel<<<dim3(pairs, CP_PARTS), CP_THREADS, 0, st>>>((const char*)d_slots, plan, n_slots, S,
                                                                          move_trees ? 1 : 0, (char*)w.puct, w.pend);
    rc = gz_check_launch("puct_compact_move_kernel");
    if (rc) return rc;
    puct_compact_swap_kernel<<<dim3(pairs, CP_PARTS), CP_THREADS, 0, st>>>((char*)d_slots, plan, n_slots);
    return gz_check_launch("puct_compact_swap_kernel");
}

}  // extern "C"
