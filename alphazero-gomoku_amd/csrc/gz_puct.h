// gz_puct.h -- what the PUCT units (gz_puct.hip, gz_puct_compact.hip, gz_puct_match.hip)
// share: the workspace layouts, each written once, the tree view of the kernels, the host
// carving of the round buffers and of the self-play prefix, the argument checks and the
// few host steps of the search that the match borrows.  Only those units include it.
//
// Workspace (gz_puct_workspace_bytes(n, S), M = S+1 nodes per game):
//   [0, 256)            PuctCfg (c_puct, seed, temp_plies, S, flags, alpha, eps, F, p, forced_k), written
//                       by gz_puct_begin (forced_k only with forced playouts, and only then read)
//   n x game_stride     per game, game_stride = al256(128 + 2334 M):
//        PuctHdr  128 B   root position, game id, node count, pending node, ...
//        W        f64 [M]
//        prior    f64 [M][225]   the evaluator's row, copied by the backup step
//        visits   i32 [M]
//        value    f32 [M]        the value the network returned for the node
//        board    u32 [M][16]    black[8], white[8] of the node's position
//        child    i16 [M][225]   -1 = none
//        parent   i16 [M]
//        move     u8  [M]        row-major cell (255 for the root)
//        term     u8  [M]        0 live, 1/2 winner colour, 3 draw (as Tree.term)
//   the round buffers (rows_bytes(n)): leaves u32 [n][16], active i32 [n], logits f32
//   [n][225], probs f32 [n][225], value f32 [n], prior f64 [n][225], every part al256, then
//   gz_pv_workspace_bytes(n) for the forward.
// About 2.3 KB per node: 1.9 GB at 4096 games x 200 simulations.  node_width below is that
// record; every offset, the export and compaction's copy are derived from it.
//
// Export (gz_puct_trees, gz_puct_tree_bytes(S) = al256(16 + 1884 M) per game):
//   i32 n_nodes, n_evals, main_draws, move; then W, prior, visits, value, board,
//   parent, move, term as above (no child table), nodes in creation order.
//
// Batched workspace (gz_puct_batch_workspace_bytes(n, S, K)): PuctCfg and the trees as
// above, then pend i16 [n][K] (the node of every active row), 256 bytes for the
// remaining count, the round buffers and the forward's workspace for n K rows.
//
// Self-play workspace (gz_selfplay_puct_workspace_bytes(n, S); gz_selfplay_puct_layout gives
// the offsets), every part al256: boards gz_board_state [n], game ids i64 [n], moves i32
// [n], stats gz_search_stats [n], visits i32 [n][225], root_q f64 [n], then
//   pend   u16 [n][200][225]   the visit rows of every slot's game in progress
//   the PUCT block             the workspace above for n games
// Capacity and active count (gz_selfplay_puct_run_active, gz_selfplay_puct_rounds_active):
// n is the capacity, which places every part; a run of the first n_active <= n slots
// launches n_active workgroups, forwards n_active (K) rows and leaves the rest alone --
// the per-slot indexing (tree_of, pend + s 200 225, leaf row s) is the same either way.
//
// Gumbel root (GZ_PUCT_GUMBEL, gz_gumbel.h): behind the flag-clear size (and behind the leaf
// symmetry's bytes, rounded up to 256, when that flag is set too), gz_puct_gumbel_bytes(n, S,
// max_considered): gs f64 [n][225], every part al256, then the tables seq(m', S), m' = 1 ..
// max_considered, int16 [max_considered][S], written by gz_puct_begin.
//
// Match workspace (gz_puct_match_workspace_bytes(n, S)): the self-play workspace of n slots,
// then side i32 [n], row_of i32 [n], the counts (256 bytes) and per side the round buffers of
// n rows (leaves, an unused active column, logits, probs, value, prior, the forward's scratch).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "gz_forced.h"
#include "gz_gumbel.h"
#include "gz_internal.h"
#include "gz_search.h"

namespace gz {

__host__ __device__ constexpr size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

inline hipStream_t as_stream(void* s) { return (hipStream_t)s; }

struct PuctCfg {
    double c_puct;
    uint64_t seed;
    int32_t temp_plies;
    int32_t S;
    int32_t flags;  // GZ_PUCT_ROOT_NOISE | GZ_PUCT_PLAYOUT_CAP
    int32_t leaves;  // K of a batched search (GZ_PUCT_LEAF_BATCH), 0: one leaf per round
    double noise_alpha;
    double noise_eps;
    int32_t fast;      // F of GZ_PUCT_PLAYOUT_CAP
    int32_t pad;
    double full_prob;  // p
    double forced_k;   // k > 0 of GZ_PUCT_FORCED_PLAYOUTS: written and read by the forced kernels only
};
static_assert(sizeof(PuctCfg) <= 256, "the configuration block");

// The root noise of a launch, by value.  on: 0 none, 1 mix with (seed, alpha, eps),
// -1 as gz_puct_begin stored it in the workspace's PuctCfg (gz_puct_backup and
// gz_puct_reroot take no params).
struct PuctNoise {
    double alpha;
    double eps;
    uint64_t seed;
    int32_t on;
    int32_t pad;
};

// The playout cap of a launch, by value.  on: 0 none (every root is full, budget S), 1 cap
// with (fast, full_prob), -1 as gz_puct_begin stored it in the workspace's PuctCfg.
struct PuctCap {
    double full_prob;
    int32_t fast;
    int32_t on;
};

struct PuctHdr {  // 128 bytes
    uint32_t black[8];
    uint32_t white[8];
    int64_t game_id;
    int32_t n_moves;
    int32_t player;
    int32_t over;        // the root is finished (or full): no search, move -1
    int32_t n_nodes;
    int32_t n_evals;     // nodes the evaluator was asked for
    int32_t main_draws;  // draws on the (game, ply, 0) stream (0 or 1)
    int32_t pending;     // node waiting for its prior and value, -1 = none
    int32_t move;
    int32_t new_evals;   // evaluations since the last move (gz_selfplay_puct_rounds' slot statistics)
    int32_t reuse;       // REUSE_MAGIC: a tree of gz_selfplay_puct_rounds (0: gz_puct_begin, a reset)
    int32_t rounds;      // rounds of gz_selfplay_puct_rounds since the last move
    int32_t budget;      // B: the search is finished at B + 1 root visits (S, or F on a fast ply)
    int32_t full;        // a full ply (always without GZ_PUCT_PLAYOUT_CAP): its root row takes the noise
    int32_t pad[1];
};
constexpr int32_t REUSE_MAGIC = 0x52455553;
static_assert(sizeof(PuctHdr) == 128, "puct header");

// ---------------------------------------------------------------- the node record
// Bytes per node of every per-game array, in the order the arrays lie behind the PuctHdr.
enum NodeField { NF_W, NF_PRIOR, NF_VISITS, NF_VALUE, NF_BOARD, NF_CHILD, NF_PARENT, NF_MOVE, NF_TERM, NODE_FIELDS };

__host__ __device__ constexpr size_t node_width(int f) {
    constexpr int NODE_WIDTH[NODE_FIELDS] = {8, 8 * GZ_CELLS, 4, 4, 64, 2 * GZ_CELLS, 2, 1, 1};
    return NODE_WIDTH[f];
}

// the bytes per node in front of field f (f = NODE_FIELDS: of the whole record)
__host__ __device__ constexpr size_t node_offset(int f) {
    size_t off = 0;
    for (int a = 0; a < f; a++) off += node_width(a);
    return off;
}

constexpr size_t NODE_BYTES = node_offset(NODE_FIELDS);
// the export: W .. board, then parent .. term (no child table), behind 16 bytes of header words
constexpr size_t EXPORT_HEAD_BYTES = node_offset(NF_CHILD);
constexpr size_t EXPORT_TAIL_OFFSET = node_offset(NF_PARENT);
constexpr size_t EXPORT_TAIL_BYTES = NODE_BYTES - EXPORT_TAIL_OFFSET;
constexpr size_t EXPORT_NODE_BYTES = EXPORT_HEAD_BYTES + EXPORT_TAIL_BYTES;
static_assert(NODE_BYTES == 2334 && EXPORT_NODE_BYTES == 1884, "the node record and its export");
static_assert(EXPORT_HEAD_BYTES == 1880 && EXPORT_TAIL_OFFSET == 2330 && EXPORT_TAIL_BYTES == 4, "the export's spans");
static_assert(EXPORT_HEAD_BYTES % 4 == 0, "the export copies W .. board as 4-byte words");

__host__ __device__ inline size_t game_stride_for(int S) {
    return al256(sizeof(PuctHdr) + NODE_BYTES * ((size_t)S + 1));
}

__host__ __device__ inline size_t export_bytes_for(int S) { return al256(16 + EXPORT_NODE_BYTES * ((size_t)S + 1)); }

struct PuctTree {
    PuctHdr* h;
    double* W;
    double* prior;
    int32_t* visits;
    float* value;
    uint32_t* board;
    int16_t* child;
    int16_t* parent;
    uint8_t* move;
    uint8_t* term;
};

__device__ inline PuctTree tree_of(char* ws, int g, int S) {
    const size_t M = (size_t)S + 1;
    char* h = ws + 256 + (size_t)g * game_stride_for(S);
    const auto at = [=](int f) { return h + sizeof(PuctHdr) + node_offset(f) * M; };
    return {(PuctHdr*)h,           (double*)at(NF_W),      (double*)at(NF_PRIOR),   (int32_t*)at(NF_VISITS),
            (float*)at(NF_VALUE),  (uint32_t*)at(NF_BOARD), (int16_t*)at(NF_CHILD), (int16_t*)at(NF_PARENT),
            (uint8_t*)at(NF_MOVE), (uint8_t*)at(NF_TERM)};
}

// a tree of gz_selfplay_puct_rounds whose root is the slot's game and position
__device__ inline bool tree_matches(const PuctHdr* h, const SlotHeader* sh) {
    const int lane = lane_id();
    bool ne = false;
    if (lane < 16) ne = ((const uint32_t*)h)[lane] != ((const uint32_t*)sh)[lane];  // black[8], white[8] in both
    return ballot(ne) == 0 && h->reuse == REUSE_MAGIC && h->game_id == sh->game_id && h->n_moves == sh->n_moves;
}

__device__ inline const SlotHeader* slot_of(const char* slots, int s) {
    return (const SlotHeader*)(slots + (size_t)s * slot_stride_bytes());
}

// One tile of a one-workgroup scan over slots, 1024 threads, one slot each: the thread's
// rank among the threads of the tile with x set, and among those with y set, both in
// ascending thread order and on top of carry[0..1], which then move past the tile.  Every
// thread of the workgroup calls; carry is the caller's LDS, zeroed (and synchronised)
// before the first tile.
__device__ inline void rank_two_classes(bool x, bool y, int* carry, int& rank_x, int& rank_y) {
    __shared__ int wsum[2][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t mx = __ballot(x), my = __ballot(y);
    if (lane == 0) {
        wsum[0][wave] = __popcll(mx);
        wsum[1][wave] = __popcll(my);
    }
    __syncthreads();
    int bx = carry[0], by = carry[1];
    for (int w = 0; w < wave; w++) {
        bx += wsum[0][w];
        by += wsum[1][w];
    }
    const uint64_t below = (1ull << lane) - 1;
    rank_x = bx + __popcll(mx & below);
    rank_y = by + __popcll(my & below);
    __syncthreads();
    if (tid == 0) {
        for (int w = 0; w < 16; w++) {
            carry[0] += wsum[0][w];
            carry[1] += wsum[1][w];
        }
    }
    __syncthreads();
}

// ---------------------------------------------------------------- the round buffers
// A block of parts, part a holding `count` elements of width[a] bytes, every part al256: the
// bytes in front of part i (i = the number of parts: of the whole block).
inline size_t part_offset(const size_t* width, size_t count, int i) {
    size_t off = 0;
    for (int a = 0; a < i; a++) off += al256(count * width[a]);
    return off;
}

struct RoundBufs {
    uint32_t* leaves;
    int32_t* active;
    float *logits, *probs, *value;
    double* prior;
    void* pvws;
};
// bytes per row of RoundBufs' parts, in its order; pvws is what follows them
constexpr int ROW_PARTS = 6;
constexpr size_t ROW_WIDTH[ROW_PARTS] = {64, 4, 4 * GZ_CELLS, 4 * GZ_CELLS, 4, 8 * GZ_CELLS};

// the round buffers of `rows` rows from p on
inline RoundBufs carve_rows(char* p, size_t rows) {
    const auto at = [=](int i) { return p + part_offset(ROW_WIDTH, rows, i); };
    return {(uint32_t*)at(0), (int32_t*)at(1), (float*)at(2), (float*)at(3), (float*)at(4), (double*)at(5), at(ROW_PARTS)};
}

// a block of round buffers with the forward's workspace behind them
inline size_t rows_bytes(size_t rows) {
    return part_offset(ROW_WIDTH, rows, ROW_PARTS) + gz_pv_workspace_bytes((int32_t)rows);
}

inline size_t rounds_offset(int32_t n, int32_t S) { return 256 + (size_t)n * game_stride_for(S); }

// (n: the game count the workspace was sized for -- a search of fewer games on it finds
// every buffer where the full one does)
inline RoundBufs carve_rounds(void* ws, int32_t n, int32_t S) { return carve_rows((char*)ws + rounds_offset(n, S), n); }

// ---------------------------------------------------------------- the self-play prefix
struct SelfplayWs {
    gz_board_state* boards;
    int64_t* gids;
    int32_t* moves;
    gz_search_stats* stats;
    int32_t* visits;
    double* root_q;
    uint16_t* pend;
    void* puct;
};

// bytes per slot of SelfplayWs' parts, in its order; the PUCT block is what follows them
constexpr int SELFPLAY_PARTS = 7;
constexpr size_t SELFPLAY_WIDTH[SELFPLAY_PARTS] = {sizeof(gz_board_state), 8, 4, sizeof(gz_search_stats),
                                                   4 * GZ_CELLS,           8, (size_t)GZ_MAX_GAME_PLIES * GZ_CELLS * 2};

inline size_t selfplay_head_bytes(int32_t n) { return part_offset(SELFPLAY_WIDTH, n, SELFPLAY_PARTS); }

inline SelfplayWs carve_selfplay(void* ws, int32_t n) {
    const auto at = [=](int i) { return (char*)ws + part_offset(SELFPLAY_WIDTH, n, i); };
    return {(gz_board_state*)at(0), (int64_t*)at(1), (int32_t*)at(2),  (gz_search_stats*)at(3),
            (int32_t*)at(4),        (double*)at(5),  (uint16_t*)at(6), at(SELFPLAY_PARTS)};
}

// ---------------------------------------------------------------- leaf symmetry
// GZ_PUCT_LEAF_SYM (gz_sym.h, gz_pvsym.hip): t is the extra region behind the flag-clear
// workspace, gz_puct_sym_bytes(rows): one byte per row of the round buffers; nullptr with the
// flag clear, and then neither step launches anything.  sym_leaves turns the round's leaf rows in place -- the
// select, begin and round kernels rewrite every row of every round and nothing but the
// forward reads the buffer (the backup kernels take no leaf pointer; a node's board is in
// its tree) -- and sym_priors maps the forward's prior rows back before the backup, which
// reads nothing else of the 225-wide buffers.
struct LeafSym {
    uint8_t* t;
    uint64_t seed;
};

inline LeafSym leaf_sym(const gz_puct_params* p, void* ws, size_t flag_clear_bytes) {
    LeafSym ls;
    ls.t = (p->flags & GZ_PUCT_LEAF_SYM) ? (uint8_t*)ws + flag_clear_bytes : nullptr;
    ls.seed = p->seed;
    return ls;
}

inline int sym_leaves(const LeafSym& ls, uint32_t* leaves, int32_t rows, void* stream) {
    if (!ls.t) return GZ_OK;
    return gz_internal_sym_boards(leaves, leaves, rows, nullptr, nullptr, ls.seed, ls.t, stream);
}

inline int sym_priors(const LeafSym& ls, double* prior, int32_t rows, void* stream) {
    if (!ls.t) return GZ_OK;
    return gz_internal_sym_rows(nullptr, nullptr, prior, rows, nullptr, ls.t, stream);
}

// ---------------------------------------------------------------- argument checks
inline int check_S(const char* who, int32_t n, int32_t S) {
    if (S < 1 || S > GZ_MAX_SIMULATIONS)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": num_simulations out of range [1, 4095]");
    if (n < 0) return gz_fail(GZ_ERR_ARG, std::string(who) + ": n < 0");
    return GZ_OK;
}

inline int check_alpha(const char* who, double alpha) {
    if (!(alpha >= 1e-3 && alpha <= 1e3))  // (a NaN fails both)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": noise alpha must be finite and in [1e-3, 1e3]");
    return GZ_OK;
}

// The root noise p asks for.  Only with GZ_PUCT_ROOT_NOISE set is p a
// gz_puct_noise_params; without it nothing past the 32 bytes of gz_puct_params is read.
inline int read_noise(const char* who, const gz_puct_params* p, PuctNoise& nz) {
    nz.alpha = 0.0;
    nz.eps = 0.0;
    nz.seed = p->seed;
    nz.on = 0;
    nz.pad = 0;
    if (!(p->flags & GZ_PUCT_ROOT_NOISE)) return GZ_OK;
    const gz_puct_noise_params* q = (const gz_puct_noise_params*)p;
    int rc = check_alpha(who, q->noise_alpha);
    if (rc) return rc;
    if (!(q->noise_eps >= 0.0 && q->noise_eps <= 1.0))
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": noise eps must be in [0, 1]");
    nz.alpha = q->noise_alpha;
    nz.eps = q->noise_eps;
    nz.on = 1;
    return GZ_OK;
}

// The forced playouts p asks for: k = 0 without GZ_PUCT_FORCED_PLAYOUTS (nothing past the cap
// struct is read then), else gz_puct_forced_params.forced_k, finite and in [0, 16].  k = 0
// with the flag forces and prunes nothing: every path treats it as the flag clear.
inline int read_forced(const char* who, const gz_puct_params* p, double& k) {
    k = 0.0;
    if (!(p->flags & GZ_PUCT_FORCED_PLAYOUTS)) return GZ_OK;
    if (p->flags & GZ_PUCT_LEAF_BATCH)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": forced playouts with leaf batching are not supported");
    const double x = ((const gz_puct_forced_params*)p)->forced_k;
    if (!forced_k_ok(x)) return gz_fail(GZ_ERR_ARG, std::string(who) + ": forced_k must be finite and in [0, 16]");
    k = x > 0.0 ? x : 0.0;  // (-0.0: 0.0)
    return GZ_OK;
}

// The Gumbel root of a search, by value (on: 0 none).  gs and seq: the extra region of the
// workspace (gumbel_region).
struct PuctGumbel {
    double c_visit, c_scale, gumbel_scale;
    uint64_t seed;
    double* gs;      // [n][225]
    int16_t* seq;    // [max_considered][S]
    int32_t max_considered;
    int32_t on;
};

// The Gumbel root p asks for.  Only with GZ_PUCT_GUMBEL set is p a gz_puct_gumbel_params;
// without it nothing past the forced struct is read.  gs and seq are left null.
inline int read_gumbel(const char* who, const gz_puct_params* p, PuctGumbel& gm) {
    gm = PuctGumbel{};
    gm.seed = p->seed;
    if (!(p->flags & GZ_PUCT_GUMBEL)) return GZ_OK;
    if (p->flags & (GZ_PUCT_ROOT_NOISE | GZ_PUCT_LEAF_BATCH | GZ_PUCT_PLAYOUT_CAP | GZ_PUCT_FORCED_PLAYOUTS))
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": the Gumbel root with root noise, leaf batching, the playout "
                                                      "cap or forced playouts is not supported");
    const gz_puct_gumbel_params* q = (const gz_puct_gumbel_params*)p;
    if (!gumbel_args_ok(q->max_considered, q->c_visit, q->c_scale, q->gumbel_scale))
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": the Gumbel root needs max_considered in [1, 32], c_visit in "
                                                      "[0, 1e4], c_scale in [0, 1e3] and gumbel_scale in [0, 8]");
    gm.c_visit = q->c_visit;
    gm.c_scale = q->c_scale;
    gm.gumbel_scale = q->gumbel_scale;
    gm.max_considered = q->max_considered;
    gm.on = 1;
    return GZ_OK;
}

static_assert(GZ_GUMBEL_MAX_CONSIDERED == GZ_PUCT_GUMBEL_MAX_CONSIDERED && GZ_GUMBEL_ROW_SCALE == GZ_PUCT_GUMBEL_ROW_SCALE,
              "gz_gumbel.h and gzero.h name the same limits");

inline size_t gumbel_gs_bytes(int32_t n) { return al256((size_t)n * GZ_CELLS * sizeof(double)); }

// gs and seq of a workspace carved for n_cap games: behind the flag-clear size, and behind the
// leaf symmetry's bytes when p sets that flag too
inline void gumbel_region(PuctGumbel& gm, const gz_puct_params* p, void* ws, int32_t n_cap) {
    size_t off = gz_puct_workspace_bytes(n_cap, p->num_simulations);
    if (p->flags & GZ_PUCT_LEAF_SYM) off += gz_puct_sym_bytes(n_cap);
    off = al256(off);
    gm.gs = (double*)((char*)ws + off);
    gm.seq = (int16_t*)((char*)ws + off + gumbel_gs_bytes(n_cap));
}

inline bool known_precision(int32_t x) { return x == GZ_PV_FP32 || x == GZ_PV_F16X3 || x == GZ_PV_F16; }

// the buffers and counts of a self-play entry point (count: its plies or rounds)
inline int check_selfplay_args(const char* who, const void* d_slots, int32_t n_slots, int32_t count,
                               const void* d_counters, const void* d_records, int32_t record_cap,
                               const void* d_workspace, bool weights, const void* d_visits) {
    if (!d_slots || n_slots <= 0 || count < 0 || !d_counters || !d_records || record_cap < 0 || !d_workspace ||
        !weights || !d_visits)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": bad arguments");
    return GZ_OK;
}

inline int check_active(const char* who, int32_t n, int32_t n_slots) {
    if (n < 1 || n > n_slots) return gz_fail(GZ_ERR_ARG, std::string(who) + ": n_active out of range [1, n_slots]");
    return GZ_OK;
}

// ---------------------------------------------------------------- host steps of gz_puct.hip
// What gz_puct_match_run borrows besides the public gz_puct_select.  C++ linkage: a
// declaration that drifts from its definition fails to link.
// gz_puct_begin on a workspace carved for n_cap games, of which the first n begin
int gz_internal_puct_begin(const gz_board_state* d_boards, const int64_t* d_game_ids, int32_t n_cap, int32_t n,
                           const gz_puct_params* p, void* d_workspace, uint32_t* d_leaves, int32_t* d_active,
                           void* stream);
int gz_internal_puct_backup(void* ws, int32_t n, int32_t S, const double* d_prior, const float* d_value,
                            const PuctNoise& nz, void* stream);
int gz_internal_puct_finish(void* ws, int32_t n, int32_t S, int32_t* d_moves, int32_t* d_visits, double* d_root_q,
                            gz_search_stats* d_stats, void* stream);
// the end of a lock-step ply: the search's visit rows into pend, then the commit of the moves
int gz_internal_puct_stash_commit(void* d_slots, int32_t n, const SelfplayWs& w, gz_record* d_records,
                                  int32_t record_cap, uint16_t* d_visits, gz_selfplay_counters* d_counters,
                                  void* stream);

}  // namespace gz
