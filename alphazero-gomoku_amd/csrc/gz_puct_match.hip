// gz_puct_match.hip -- the match: two networks play each other in one device-side loop
// (gz_puct_match_run, gz_puct_match_results; tests/puct_match_ref.py restates it).
//
// The lock-step self-play ply with two evaluators.  Side A (0) plays black in game g iff
// ((g ^ parity) & 1) == 0, and the side that moves at a search's root evaluates every leaf
// of that search.  Per ply, after the boards:
//   1. puct_match_plan_kernel     one workgroup: side[s] (-1: idle, its board marked over, so
//                                 begin gives it no leaf and finish move -1), row_of[s] = the
//                                 slot's rank among its side's slots in ascending slot order,
//                                 count[0..1];
//   2. per round (S+1), between select and backup:
//        puct_match_gather_kernel   leaf row s -> packed leaves of side[s], row row_of[s];
//        gz_pv_forward x 2          side i's blob and precision over count[i] rows (the count
//                                   is read on the device; a count of 0 evaluates nothing);
//        puct_match_scatter_kernel  packed prior row and value -> slot row s of the round
//                                   buffers, which backup reads as ever;
//   3. finish, stash, commit as gz_selfplay_puct_run.
// With GZ_PUCT_LEAF_SYM the slot rows turn before the gather and turn back after the scatter,
// so both sides see the same t and a round still has two extra launches.
// The search itself -- begin, select, backup, finish, stash and commit -- is gz_puct.hip's.
#include "gz_puct.h"

using namespace gz;

namespace {

__device__ inline int match_side(int64_t game_id, int player, int parity) {
    const bool a_black = (((int)(game_id & 1) ^ parity) & 1) == 0;
    return (player == 1) == a_black ? 0 : 1;
}

// Once per ply, one workgroup over the first n slots in tiles of 1024 (rank_two_classes):
// side[s] = the mover's side or -1 for an idle slot, row_of[s] = the slot's rank among the
// slots of its side in ascending slot order, count[0..1] = the slots per side.  An idle
// slot's board is marked over, so the search leaves it alone (no leaf, no backup, move -1)
// whatever its prior and value rows hold.
__global__ __launch_bounds__(1024) void puct_match_plan_kernel(const char* slots, int n, int parity,
                                                               gz_board_state* boards, int32_t* side,
                                                               int32_t* row_of, int32_t* count) {
    __shared__ int carry[2];
    const int tid = threadIdx.x;
    if (tid == 0) carry[0] = carry[1] = 0;
    __syncthreads();
    for (int t0 = 0; t0 < n; t0 += 1024) {
        const int s = t0 + tid;
        int sd = -1;
        if (s < n) {
            const SlotHeader* h = slot_of(slots, s);
            if (h->game_id < h->game_id_end) sd = match_side(h->game_id, h->player, parity);
            else boards[s].over = 1;
        }
        int r0, r1;
        rank_two_classes(sd == 0, sd == 1, carry, r0, r1);
        if (s < n) {
            side[s] = sd;
            row_of[s] = sd == 0 ? r0 : (sd == 1 ? r1 : 0);
        }
    }
    if (tid < 2) count[tid] = carry[tid];
}

// leaf row s (64 bytes, four 16-byte words) -> row row_of[s] of its side's packed leaves
__global__ __launch_bounds__(256) void puct_match_gather_kernel(const uint32_t* leaves, int n, const int32_t* side,
                                                                const int32_t* row_of, uint32_t* packed0,
                                                                uint32_t* packed1) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int s = i >> 2, q = i & 3;
    if (s >= n) return;
    const int sd = side[s];
    if (sd < 0) return;
    uint4* dst = (uint4*)(sd == 0 ? packed0 : packed1);
    dst[(size_t)row_of[s] * 4 + q] = ((const uint4*)leaves)[(size_t)s * 4 + q];
}

// One wave per slot: row row_of[s] of its side's packed prior (225 fp64) and value -> slot
// row s of the round buffers (rows are 1800 bytes apart: 8-byte words).
__global__ __launch_bounds__(256) void puct_match_scatter_kernel(int n, const int32_t* side, const int32_t* row_of,
                                                                 const double* prior0, const double* prior1,
                                                                 const float* value0, const float* value1,
                                                                 double* prior, float* value) {
    const int s = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (s >= n) return;
    const int sd = side[s];
    if (sd < 0) return;
    const size_t r = (size_t)row_of[s];
    const double* src = (sd == 0 ? prior0 : prior1) + r * GZ_CELLS;
    double* dst = prior + (size_t)s * GZ_CELLS;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (lane + WAVE * k < GZ_CELLS) dst[lane + WAVE * k] = src[lane + WAVE * k];
    if (lane == 0) value[s] = (sd == 0 ? value0 : value1)[r];
}

// gz_puct_match_results: one thread per record
__global__ __launch_bounds__(256) void puct_match_results_kernel(const gz_record* records, int n, int parity,
                                                                 int64_t base, int n_games,
                                                                 gz_puct_match_tally* tally, int8_t* result) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool in = i < n;
    int first = 0, res = 0, a_black = 0;
    if (in) {
        const gz_record& r = records[i];
        if (r.ply == 0) {  // the mover is black, z black's result
            first = 1;
            a_black = match_side(r.game_id, 1, parity) == 0;
            res = a_black ? r.z : -r.z;
            const int64_t k = r.game_id - base;
            if (result && k >= 0 && k < n_games) result[k] = (int8_t)res;
        }
    }
    // (one atomic per wave and field)
    unsigned long long* t = (unsigned long long*)tally;
    const unsigned long long c[9] = {
        (unsigned long long)__popcll(__ballot(first)),
        (unsigned long long)__popcll(__ballot(first && res > 0)),
        (unsigned long long)__popcll(__ballot(first && res < 0)),
        (unsigned long long)__popcll(__ballot(first && res == 0)),
        (unsigned long long)__popcll(__ballot(first && res > 0 && a_black)),
        (unsigned long long)__popcll(__ballot(first && res > 0 && !a_black)),
        (unsigned long long)__popcll(__ballot(first && res < 0 && !a_black)),
        (unsigned long long)__popcll(__ballot(first && res < 0 && a_black)),
        (unsigned long long)__popcll(__ballot(in))};
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int f = 0; f < 9; f++)
            if (c[f]) atomicAdd(t + f, c[f]);
    }
}

// the match workspace after the self-play workspace of n slots: side i32 [n], row_of i32
// [n], the two counts (256 bytes), then per side the round buffers of n rows
struct MatchWs {
    int32_t *side, *row_of, *count;
    RoundBufs pk[2];
};

MatchWs carve_match(void* ws, int32_t n, int32_t S) {
    char* p = (char*)ws + gz_selfplay_puct_workspace_bytes(n, S);
    MatchWs m;
    m.side = (int32_t*)p;
    p += al256((size_t)n * 4);
    m.row_of = (int32_t*)p;
    p += al256((size_t)n * 4);
    m.count = (int32_t*)p;
    p += 256;
    m.pk[0] = carve_rows(p, n);
    p += rows_bytes(n);
    m.pk[1] = carve_rows(p, n);
    return m;
}

}  // namespace

extern "C" {

size_t gz_puct_match_workspace_bytes(int32_t n_slots, int32_t S) {
    if (n_slots < 1) n_slots = 1;
    return gz_selfplay_puct_workspace_bytes(n_slots, S) + 2 * al256((size_t)n_slots * 4) + 256 + 2 * rows_bytes(n_slots);
}

// gz_selfplay_puct_run's ply with the routed evaluation in place of the one forward
int gz_puct_match_run(void* d_slots, int32_t n_slots, int32_t n, const gz_puct_match_params* mp, void* d_workspace,
                      int32_t n_plies, gz_record* d_records, int32_t record_cap, uint16_t* d_visits,
                      gz_selfplay_counters* d_counters, void* stream) {
    const char* who = "gz_puct_match_run";
    if (!mp || !mp->search) return gz_fail(GZ_ERR_ARG, std::string(who) + ": params is NULL");
    const gz_puct_params* p = mp->search;
    int rc = check_S(who, n_slots, p->num_simulations);
    if (rc) return rc;
    if (p->flags & GZ_PUCT_LEAF_BATCH)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": leaf batching is not supported in a match");
    if (p->flags & GZ_PUCT_PLAYOUT_CAP)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": the playout cap is not supported in a match");
    if (p->flags & GZ_PUCT_FORCED_PLAYOUTS)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": forced playouts are not supported in a match");
    if (p->flags & GZ_PUCT_GUMBEL)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": the Gumbel root is not supported in a match");
    PuctNoise nz;
    rc = read_noise(who, p, nz);
    if (rc) return rc;
    if (!known_precision(mp->precision[0]) || !known_precision(mp->precision[1]))
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": unknown precision");
    if (mp->a_black_parity != 0 && mp->a_black_parity != 1)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": a_black_parity must be 0 or 1");
    rc = check_selfplay_args(who, d_slots, n_slots, n_plies, d_counters, d_records, record_cap, d_workspace,
                             mp->d_weights[0] && mp->d_weights[1], d_visits);
    if (rc) return rc;
    rc = check_active(who, n, n_slots);
    if (rc) return rc;
    const int S = p->num_simulations;
    const SelfplayWs w = carve_selfplay(d_workspace, n_slots);
    const RoundBufs r = carve_rounds(w.puct, n_slots, S);
    const MatchWs m = carve_match(d_workspace, n_slots, S);
    const LeafSym ls = leaf_sym(p, d_workspace, gz_puct_match_workspace_bytes(n_slots, S));
    hipStream_t st = as_stream(stream);
    for (int it = 0; it < n_plies; it++) {
        rc = gz_selfplay_boards(d_slots, n, S, w.boards, w.gids, stream);
        if (rc) return rc;
        puct_match_plan_kernel<<<1, 1024, 0, st>>>((const char*)d_slots, n, mp->a_black_parity, w.boards, m.side,
                                                   m.row_of, m.count);
        rc = gz_check_launch("puct_match_plan_kernel");
        if (rc) return rc;
        rc = gz_internal_puct_begin(w.boards, w.gids, n_slots, n, p, w.puct, r.leaves, r.active, stream);
        if (rc) return rc;
        for (int round = 0; round <= S; round++) {
            if (round > 0) {
                rc = gz_puct_select(w.puct, n, S, r.leaves, r.active, stream);
                if (rc) return rc;
            }
            rc = sym_leaves(ls, r.leaves, n, stream);
            if (rc) return rc;
            puct_match_gather_kernel<<<(n * 4 + 255) / 256, 256, 0, st>>>(r.leaves, n, m.side, m.row_of,
                                                                          m.pk[0].leaves, m.pk[1].leaves);
            rc = gz_check_launch("puct_match_gather_kernel");
            if (rc) return rc;
            for (int sd = 0; sd < 2; sd++) {
                const RoundBufs& k = m.pk[sd];
                rc = gz_pv_forward(mp->d_weights[sd], k.leaves, n, m.count + sd, k.logits, k.value, k.probs,
                                   k.prior, k.pvws, mp->precision[sd], stream);
                if (rc) return rc;
            }
            puct_match_scatter_kernel<<<(n + 3) / 4, 256, 0, st>>>(n, m.side, m.row_of, m.pk[0].prior, m.pk[1].prior,
                                                                   m.pk[0].value, m.pk[1].value, r.prior, r.value);
            rc = gz_check_launch("puct_match_scatter_kernel");
            if (rc) return rc;
            rc = sym_priors(ls, r.prior, n, stream);
            if (rc) return rc;
            rc = gz_internal_puct_backup(w.puct, n, S, r.prior, r.value, nz, stream);
            if (rc) return rc;
        }
        rc = gz_internal_puct_finish(w.puct, n, S, w.moves, w.visits, w.root_q, w.stats, stream);
        if (rc) return rc;
        rc = gz_internal_puct_stash_commit(d_slots, n, w, d_records, record_cap, d_visits, d_counters, stream);
        if (rc) return rc;
    }
    return GZ_OK;
}

int gz_puct_match_results(const gz_record* d_records, int32_t n_records, int32_t a_black_parity,
                          int64_t game_id_base, int32_t n_games, gz_puct_match_tally* d_tally, int8_t* d_result,
                          void* stream) {
    if (n_records < 0 || n_games < 0 || !d_tally || (n_records > 0 && !d_records))
        return gz_fail(GZ_ERR_ARG, "gz_puct_match_results: bad arguments");
    if (a_black_parity != 0 && a_black_parity != 1)
        return gz_fail(GZ_ERR_ARG, "gz_puct_match_results: a_black_parity must be 0 or 1");
    if (n_records == 0) return GZ_OK;
    puct_match_results_kernel<<<(n_records + 255) / 256, 256, 0, as_stream(stream)>>>(
        d_records, n_records, a_black_parity, game_id_base, n_games, d_tally, d_result);
    return gz_check_launch("puct_match_results_kernel");
}

}  // extern "C"
