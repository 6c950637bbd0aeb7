// gz_puct.hip -- network-guided PUCT search (the opt-in "puct" search mode).
//
// The default mode reproduces the reference's search, in which MCTSNode.prior_prob
// is written and never read and the value head is never consulted.  Here the
// priors steer selection (PUCT) and the value head replaces the rollout; self-play
// emits the root's visit counts as the policy target.
//
// One 64-lane wavefront (one workgroup) owns one game.  Lane l owns the cells l,
// l+64, l+128 and l+192 (the last chunk has 33 valid lanes), so chunk k of a wave
// is the contiguous cell range [64k, 64k+64).  A search is S+1 lock-step rounds
// over all games, each round three stream-ordered steps:
//
//   1. puct_select_kernel  descends by PUCT from the root to a new child, creates
//                          it and puts its board into the game's leaf row (row g of
//                          [n][16]); a descent that ends in a terminal node backs
//                          its value up at once and leaves an empty board;
//   2. gz_pv_forward       over the n leaf rows (rows are fixed per game, never
//                          compacted: static launch shapes, order-independent results);
//   3. puct_backup_kernel  stores the prior row and the value in the new node and
//                          backs the value up.
//
// Round 0 evaluates the root (gz_puct_begin writes its board instead of step 1).
// Nothing synchronises the host and nothing is copied to it.
//
// Semantics (tests/puct_ref.py restates them in Python, bit for bit): v is the
// value for the side to move at node i; a node's W is from the view of the player
// who moved into it.
//
//   backup(i, v):  s = -v; while i >= 0: visits[i] += 1; W[i] += s; s = -s; i = parent[i]
//   score(c)    =  q + u,  q = n ? W[child]/n : 0.0,
//                  u = ((c_puct * prior[i][c]) * sqrt((double)visits[i])) / (1.0 + n)
//   the move    =  the first maximum of score over the empty cells, ascending
//   terminal    :  backup(j, draw ? 0.0 : -1.0)  (proper negamax, draw = 0 -- not the
//                  default mode's un-negated, draw = 0.1 backup)
//
// All score arithmetic is fp64 in exactly that order (-ffp-contract=off); the
// network's value enters as (double)float32.
//
// Root noise (opt-in, GZ_PUCT_ROOT_NOISE; gz_dirichlet.h, tests/puct_noise_ref.py): the
// root's stored row becomes (1.0 - eps) * prior + eps * eta at its empty cells, eta ~
// Dir(alpha) from the (seed, game, ply, GZ_NOISE_SIM) stream, exactly once per root: in
// puct_backup_kernel when node 0 is the pending one (a fresh root), and after the
// re-root for an inherited root (puct_reroot_kernel, puct_advance_kernel), on its
// carried row with the key of its new ply.  No other node's row is touched.
//
// Playout cap randomization (opt-in, GZ_PUCT_PLAYOUT_CAP; tests/puct_cap_ref.py restates
// it).  A root at ply n_moves is full when to_unit(draw(stream_key(seed, game, ply,
// GZ_CAP_SIM), 0)) < full_prob and fast otherwise; its budget B is S when full, else F.
// The budget and the full mark are decided when the node becomes a root -- begin_root for
// a fresh one, after reroot() for an inherited one -- and kept in the PuctHdr, which
// compaction moves byte for byte.  A search is finished when visits[0] >= B + 1 (without
// the flag B = S everywhere: the tests of before).  An inherited root may arrive with
// v >= B + 1 visits: it gets no simulation (an inactive row), its move is picked at the
// next advance step (one round) and its visit row is the inherited child visits, v - 1.
// Root noise is mixed into the rows of full roots only.  Not with leaf batching, not in
// a match.
//
// Workspace (gz_puct_workspace_bytes(n, S), M = S+1 nodes per game):
//   [0, 256)            PuctCfg (c_puct, seed, temp_plies, S, flags, alpha, eps, F, p), written
//                       by gz_puct_begin
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
//   gz_puct_search's round buffers: leaves u32 [n][16], active i32 [n], logits f32
//   [n][225], probs f32 [n][225], value f32 [n], prior f64 [n][225], then
//   gz_pv_workspace_bytes(n) for the forward.
// About 2.3 KB per node: 1.9 GB at 4096 games x 200 simulations.
//
// Tree reuse between plies (opt-in: gz_puct_reroot, gz_selfplay_puct_rounds).  A search
// ends when visits[0] == S+1.  After the move m the next ply's tree is the subtree of
// child[0][m]: reroot() keeps its nodes in creation order, renumbers them densely and
// moves every array's rows down in place (a node's new index is below its old one and
// rows are moved in ascending order, so no row is overwritten before it is read; the
// remap table lives in LDS).  W, visits, prior, value, board and term are carried bit
// for bit, so the tree is the one a search from the new root would have built from the
// same evaluations, with visits[0] of its S+1 visits already made.  In
// gz_selfplay_puct_rounds every slot keeps its own clock: a round is
//
//   1. puct_advance_kernel     a slot whose root is at budget picks its move (pick_move,
//                              as puct_finish_kernel), stashes the visit row and, unless
//                              the move ends the game, re-roots its tree under it (one
//                              workgroup of 1024 per slot; the others leave at once);
//   2. selfplay_commit_kernel  plays the move (move -1: the slot is left alone);
//   3. puct_round_kernel       a tree that is not the slot's (a new game, a reset) gives
//                              way to a fresh root from the slot header, whose board is
//                              its leaf; every other slot descends as in step 1 above;
//   4. gz_pv_forward, 5. puct_backup_kernel as above,
//
// so every live slot has exactly one leaf in every forward.  A tree belongs to a slot
// while its header says so (reuse == REUSE_MAGIC) and its root is the slot's game id,
// move count and position; gz_selfplay_puct_reset clears the mark.
//
// Export (gz_puct_trees, gz_puct_tree_bytes(S) = al256(16 + 1884 M) per game):
//   i32 n_nodes, n_evals, main_draws, move; then W, prior, visits, value, board,
//   parent, move, term as above (no child table), nodes in creation order.
//
// Leaf batching with virtual loss (opt-in, GZ_PUCT_LEAF_BATCH; tests/puct_batch_ref.py
// restates it).  Game g owns the rows g K .. g K + K - 1 of every round buffer.  Round 0
// evaluates the root in row g K.  In every later round puct_select_batch_kernel descends
// up to K times, one descent after the other: vl[x] counts the leaves of this round that
// wait below node x and enters the score as that many visits, each lost by the selector,
//   n = visits[j] + vl[j],  q = n ? (W[j] - (double)vl[j]) / (double)n : 0.0,
//   u = ((c_puct * prior[i][c]) * sqrt((double)(visits[i] + vl[i]))) / (1.0 + (double)n)
// (W - 0.0 and n + 0: K = 1 is the search above bit for bit).  A descent starts only while
// visits[0] + vl[0] <= S; one that ends in a terminal node backs up at once and takes no
// row; one that picks a node created in this round and not yet evaluated (a collision)
// changes nothing and ends the game's selection for the round; every other one creates a
// node, puts its board into the game's next row and adds 1 to vl along its path.  The
// rows left over are empty and inactive.  puct_backup_batch_kernel then stores and backs
// up the game's active rows in ascending row order (lane 0, so W sums in that order).
// vl is int16 [S+1] in LDS for the length of the select launch and never reaches global
// memory: the backup has nothing to undo and the node record keeps its 2,334 bytes.  The
// select kernel re-reads tree words that lane 0 wrote earlier in the same launch (child,
// n_nodes, term, visits and W after a terminal backup): between two descents the wave
// drains its stores and passes a workgroup-scope release / acquire (batch_sync).
// The first descent of a round never collides, so a move takes between 1 + ceil(S/K) and
// S+1 rounds; gz_puct_search reads the largest remaining count back (4 bytes) to know.
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
// Slot compaction (gz_selfplay_puct_compact; in place).  With a active slots among the
// first n_active, the holes are the idle slots below a and the fillers the active ones at
// or above a; there are equally many, and the k-th filler goes to the k-th hole (both
// ascending).  Sources (>= a) and destinations (< a) are disjoint, so all pairs move at
// once without a second copy of the trees or of pend; the slot order is not preserved.
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
//
// The match (gz_puct_match_run): the lock-step self-play ply with two evaluators.  Side A
// (0) plays black in game g iff ((g ^ parity) & 1) == 0, and the side that moves at a
// search's root evaluates every leaf of that search.  Per ply, after the boards:
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
// Match workspace (gz_puct_match_workspace_bytes(n, S)): the self-play workspace of n slots,
// then side i32 [n], row_of i32 [n], the counts (256 bytes) and per side the round buffers of
// n rows (leaves, an unused active column, logits, probs, value, prior, the forward's scratch).
//
// Leaf symmetry (opt-in, GZ_PUCT_LEAF_SYM; gz_sym.h, gz_pvsym.hip, tests/puct_sym_ref.py):
// every leaf is evaluated on its board under t = sym_of(seed, leaf row), one of the 8
// symmetries, and the prior row is mapped back; the value is a scalar.  Two launches per
// round around the forward, in all five paths:
//   select / begin / round -> sym_leaves (leaf rows in place, t per row) -> gz_pv_forward
//   -> sym_priors (the f64 prior rows in place) -> backup (the root noise as ever, on the
//   mapped-back row);
// the match turns the slot rows before the gather and maps the slot rows back after the
// scatter, so both sides see the same t and a round still has two extra launches.  The
// select, backup, re-root and compaction kernels do not know about it.  t lives behind the
// flag-clear workspace: gz_puct_sym_bytes(rows) more bytes, touched only with the flag set.
// The step API accepts the flag and ignores it (its caller evaluates: gz_pv_forward_sym).
#include <hip/hip_runtime.h>

#include <climits>
#include <mutex>
#include <string>
#include <unordered_map>

#include "gz_dirichlet.h"
#include "gz_internal.h"
#include "gz_search.h"

using namespace gz;

namespace {

__host__ __device__ constexpr size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

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

__device__ inline PuctNoise noise_of(const PuctNoise& nz, const char* ws) {
    if (nz.on >= 0) return nz;
    const PuctCfg* cfg = (const PuctCfg*)ws;
    PuctNoise r;
    r.alpha = cfg->noise_alpha;
    r.eps = cfg->noise_eps;
    r.seed = cfg->seed;
    r.on = (cfg->flags & GZ_PUCT_ROOT_NOISE) ? 1 : 0;
    r.pad = 0;
    return r;
}

// The playout cap of a launch, by value.  on: 0 none (every root is full, budget S), 1 cap
// with (fast, full_prob), -1 as gz_puct_begin stored it in the workspace's PuctCfg.
struct PuctCap {
    double full_prob;
    int32_t fast;
    int32_t on;
};

__device__ inline PuctCap cap_of(const PuctCap& cp, const char* ws) {
    if (cp.on >= 0) return cp;
    const PuctCfg* cfg = (const PuctCfg*)ws;
    PuctCap r;
    r.full_prob = cfg->full_prob;
    r.fast = cfg->fast;
    r.on = (cfg->flags & GZ_PUCT_PLAYOUT_CAP) ? 1 : 0;
    return r;
}

// the (seed, game, ply, GZ_CAP_SIM) stream decides a ply: full or fast (host and device)
constexpr int32_t GZ_CAP_SIM = 0x50434150;  // "PCAP"; simulation streams use sim <= 4095

__host__ __device__ inline bool cap_is_full(uint64_t seed, int64_t game_id, int32_t ply, double full_prob) {
    return to_unit(draw(stream_key(seed, game_id, ply, GZ_CAP_SIM), 0)) < full_prob;
}

// is the root of (game, ply) a full search?  Without the cap every root is.
__device__ inline bool root_is_full(const PuctCap& cap, uint64_t seed, int64_t game_id, int32_t ply) {
    return !cap.on || cap_is_full(seed, game_id, ply, cap.full_prob);
}

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

__host__ __device__ inline size_t game_stride_for(int S) {
    const size_t M = (size_t)S + 1;
    return al256(sizeof(PuctHdr) + 2334 * M);
}

__host__ __device__ inline size_t export_bytes_for(int S) {
    const size_t M = (size_t)S + 1;
    return al256(16 + 1884 * M);
}

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
    char* b = ws + 256 + (size_t)g * game_stride_for(S);
    PuctTree t;
    t.h = (PuctHdr*)b;
    b += sizeof(PuctHdr);
    t.W = (double*)b;
    b += 8 * M;
    t.prior = (double*)b;
    b += 1800 * M;
    t.visits = (int32_t*)b;
    b += 4 * M;
    t.value = (float*)b;
    b += 4 * M;
    t.board = (uint32_t*)b;
    b += 64 * M;
    t.child = (int16_t*)b;
    b += 450 * M;
    t.parent = (int16_t*)b;
    b += 2 * M;
    t.move = (uint8_t*)b;
    b += M;
    t.term = (uint8_t*)b;
    return t;
}

__device__ inline void backup(const PuctTree& t, int i, double v) {
    double s = -v;
    while (i >= 0) {
        t.visits[i] += 1;
        t.W[i] += s;
        s = -s;
        i = t.parent[i];
    }
}

// eta of a root with the empty cells E for this lane's cells (eta[k]: cell lane + 64 k;
// 0 at stones): every lane samples the Gamma(alpha) of its own cells, then every lane
// adds all 225 up in ascending cell order (one running fp64 sum, as the reference; a
// stone's 0.0 changes nothing) and divides.  One wave, no LDS.  false (eta all 0): the
// total is 0 or not finite.
__device__ inline bool root_eta(const BB& E, uint64_t seed, int64_t game_id, int ply, double alpha, double eta[4]) {
    const int lane = lane_id();
    const uint64_t key = stream_key(seed, game_id, ply, GZ_NOISE_SIM);
#pragma unroll
    for (int j = 0; j < 4; j++) eta[j] = 0.0;
#pragma unroll 1
    for (int k = 0; k < 4; k++) {  // (one copy of the sampler; the result goes to eta[k] by select)
        const int c = lane + WAVE * k;
        double x = 0.0;
        if (c < GZ_CELLS && bb_test(E, cell_to_bit(c))) x = noise_gamma(key, c, alpha);
#pragma unroll
        for (int j = 0; j < 4; j++) eta[j] = j == k ? x : eta[j];
    }
    double total = 0.0;
#pragma unroll
    for (int k = 0; k < 4; k++)
        for (int l = 0; l < WAVE && WAVE * k + l < GZ_CELLS; l++) total += __shfl(eta[k], l);
    const bool ok = noise_total_ok(total);
#pragma unroll
    for (int k = 0; k < 4; k++) eta[k] = ok ? eta[k] / total : 0.0;
    return ok;
}

// the mix of the root's stored prior row, once per root (one wave)
__device__ inline void mix_root_row(const PuctTree& t, const PuctNoise& nz) {
    const PuctHdr* h = t.h;
    const int lane = lane_id();
    BB black, white;
    load_bb(black, h->black);
    load_bb(white, h->white);
    const BB E = empties(black, white);
    double eta[4];
    if (!root_eta(E, nz.seed, h->game_id, h->n_moves, nz.alpha, eta)) return;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = lane + WAVE * k;
        if (c < GZ_CELLS && bb_test(E, cell_to_bit(c))) t.prior[c] = noise_mix(t.prior[c], nz.eps, eta[k]);
    }
}

// row g of the leaf buffer: the board, or the empty board when the game has no leaf
__device__ inline void write_leaf(uint32_t* leaves, int32_t* active, int g, const BB& black, const BB& white,
                                  bool live) {
    const int lane = lane_id();
    if (lane < 16) {
        uint32_t w = lane < 8 ? bb_word(black, lane) : bb_word(white, lane - 8);
        leaves[(size_t)g * 16 + lane] = live ? w : 0u;
    }
    if (lane == 0) active[g] = live ? 1 : 0;
}

// unevaluated: the node never gets an evaluation (a terminal node, the root of a board that
// is over), so no backup stores its prior row: it is zeroed here, and gz_puct_trees exports
// a row that does not depend on what the workspace held
__device__ inline void new_node(const PuctTree& t, int j, int parent, int move, int term, const BB& black,
                                const BB& white, bool unevaluated) {
    const int lane = lane_id();
    for (int c = lane; c < GZ_CELLS; c += WAVE) t.child[(size_t)j * GZ_CELLS + c] = -1;
    if (unevaluated)
        for (int c = lane; c < GZ_CELLS; c += WAVE) t.prior[(size_t)j * GZ_CELLS + c] = 0.0;
    if (lane < 16) t.board[(size_t)j * 16 + lane] = lane < 8 ? bb_word(black, lane) : bb_word(white, lane - 8);
    if (lane == 0) {
        t.parent[j] = (int16_t)parent;
        t.move[j] = (uint8_t)move;
        t.term[j] = (uint8_t)term;
        t.visits[j] = 0;
        t.W[j] = 0.0;
        t.value[j] = 0.0f;
    }
}

// a one-node tree: the root waits for its evaluation (pending 0) unless the game is over
__device__ inline void begin_root(const PuctTree& t, const BB& black, const BB& white, int64_t game_id, int n_moves,
                                  int player, bool over, int32_t reuse, int budget, bool full) {
    new_node(t, 0, -1, 255, 0, black, white, over);
    if (lane_id() == 0) {
        PuctHdr* h = t.h;
        store_bb(h->black, black);
        store_bb(h->white, white);
        h->game_id = game_id;
        h->n_moves = n_moves;
        h->player = player;
        h->over = over ? 1 : 0;
        h->n_nodes = 1;
        h->n_evals = 0;
        h->main_draws = 0;
        h->pending = over ? -1 : 0;
        h->move = -1;
        h->new_evals = 0;
        h->reuse = reuse;
        h->budget = budget;
        h->full = full ? 1 : 0;
    }
}

// the budget of an inherited root, right after reroot() (every lane of one wave calls;
// the header already holds the new ply); returns whether the ply is full
__device__ inline bool set_budget(PuctHdr* h, const PuctCap& cap, uint64_t seed, int S) {
    const bool full = root_is_full(cap, seed, h->game_id, h->n_moves);
    if (lane_id() == 0) {
        h->budget = full ? S : cap.fast;
        h->full = full ? 1 : 0;
    }
    return full;
}

// ---------------------------------------------------------------- begin
__global__ __launch_bounds__(WAVE) void puct_begin_kernel(const gz_board_state* boards, const int64_t* game_ids, int n,
                                                          gz_puct_params p, PuctNoise nz, PuctCap cap, int K,
                                                          int16_t* pend, char* ws, uint32_t* leaves,
                                                          int32_t* active) {
    const int g = blockIdx.x;
    if (g >= n) return;
    const int lane = lane_id();
    const int S = p.num_simulations;
    const int rows = K > 0 ? K : 1;  // (K = 0, pend = nullptr: the unbatched search)
    if (g == 0 && lane == 0) {
        PuctCfg* cfg = (PuctCfg*)ws;
        cfg->c_puct = p.c_puct;
        cfg->seed = p.seed;
        cfg->temp_plies = p.temp_plies;
        cfg->S = S;
        cfg->flags = (nz.on ? GZ_PUCT_ROOT_NOISE : 0) | (cap.on ? GZ_PUCT_PLAYOUT_CAP : 0);
        cfg->leaves = K;
        cfg->noise_alpha = nz.alpha;
        cfg->noise_eps = nz.eps;
        cfg->fast = cap.fast;
        cfg->pad = 0;
        cfg->full_prob = cap.full_prob;
    }
    PuctTree t = tree_of(ws, g, S);
    const gz_board_state& bs = boards[g];
    BB black, white;
    load_bb(black, bs.black);
    load_bb(white, bs.white);
    const bool over = bs.over != 0 || !bb_any(empties(black, white));
    const bool full = root_is_full(cap, p.seed, game_ids[g], bs.n_moves);
    begin_root(t, black, white, game_ids[g], bs.n_moves, bs.player, over, 0, full ? S : cap.fast, full);
    write_leaf(leaves, active, g * rows, black, white, !over);
    for (int k = 1; k < rows; k++) write_leaf(leaves, active, g * rows + k, black, white, false);
    if (pend)
        for (int k = lane; k < rows; k += WAVE) pend[(size_t)g * rows + k] = -1;
}

// ---------------------------------------------------------------- select
// One simulation's descent of game g's tree: the new leaf's board into row g, or an
// empty row (a terminal node backed up, a game that is over, waits for a backup or
// whose root already has its budget's B+1 visits -- with tree reuse, where a game can
// reach its budget before the others, and on the fast plies of a playout cap).
__device__ inline void descend(const PuctTree& t, double c_puct, int S, int g, uint32_t* leaves, int32_t* active) {
    const int lane = lane_id();
    PuctHdr* h = t.h;
    BB black, white;
    load_bb(black, h->black);
    load_bb(white, h->white);
    // (pending: the caller skipped a backup; keep the tree as it is)
    if (h->over || h->pending >= 0 || t.visits[0] > h->budget) {
        write_leaf(leaves, active, g, black, white, false);
        return;
    }
    int mover = h->player, cnt = h->n_moves;
    int i = 0;
    while (true) {
        const int tm = t.term[i];
        if (tm) {
            if (lane == 0) backup(t, i, tm == 3 ? 0.0 : -1.0);
            write_leaf(leaves, active, g, black, white, false);
            return;
        }
        const BB E = empties(black, white);
        const double sq = __builtin_sqrt((double)t.visits[i]);
        const double* pr = t.prior + (size_t)i * GZ_CELLS;
        const int16_t* ch = t.child + (size_t)i * GZ_CELLS;
        double bv = -__builtin_inf();
        int bi = INT_MAX;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = lane + WAVE * k;
            if (c < GZ_CELLS && bb_test(E, cell_to_bit(c))) {
                const int cj = ch[c];
                int nn = 0;
                double q = 0.0;
                if (cj >= 0) {
                    nn = t.visits[cj];
                    q = nn ? t.W[cj] / (double)nn : 0.0;
                }
                const double u = ((c_puct * pr[c]) * sq) / (1.0 + (double)nn);
                const double sc = q + u;
                if (sc > bv) {
                    bv = sc;
                    bi = c;
                }
            }
        }
        wave_argmax(bv, bi);
        if (bi == INT_MAX) bi = bit_to_cell(lowest_bit(E));  // only if the evaluator gave non-finite priors
        if (bi < 0 || bi >= GZ_CELLS) {  // (a live node always has an empty cell)
            write_leaf(leaves, active, g, black, white, false);
            return;
        }
        const int bit = cell_to_bit(bi);
        const int cj = ch[bi];
        if (cj >= 0) {
            if (mover == 1) bb_set(black, bit);
            else bb_set(white, bit);
            mover = 3 - mover;
            cnt++;
            i = cj;
            continue;
        }
        const int j = h->n_nodes;
        if (j > S) {  // more select steps than the workspace was sized for: no node left
            write_leaf(leaves, active, g, black, white, false);
            return;
        }
        // make_move (gomoku_board.py:84-113): five or more wins, then the full board /
        // the 200-ply cap draws
        const bool win = bb_test(threats(mover == 1 ? black : white).win, bit);
        const int ne = bb_count(E);
        if (mover == 1) bb_set(black, bit);
        else bb_set(white, bit);
        cnt++;
        const int term = win ? mover : ((ne == 1 || cnt >= GZ_MAX_GAME_PLIES) ? 3 : 0);
        new_node(t, j, i, bi, term, black, white, term != 0);
        if (lane == 0) {
            t.child[(size_t)i * GZ_CELLS + bi] = (int16_t)j;
            h->n_nodes = j + 1;
            if (term) backup(t, j, term == 3 ? 0.0 : -1.0);
            else h->pending = j;
        }
        write_leaf(leaves, active, g, black, white, term == 0);
        return;
    }
}

__global__ __launch_bounds__(WAVE) void puct_select_kernel(char* ws, int n, int S, uint32_t* leaves, int32_t* active) {
    const int g = blockIdx.x;
    if (g >= n) return;
    const PuctCfg cfg = *(const PuctCfg*)ws;
    descend(tree_of(ws, g, S), cfg.c_puct, S, g, leaves, active);
}

// ---------------------------------------------------------------- backup
// The root noise is mixed here, into the row of a root as it is stored (node 0 pending:
// gz_puct_begin's, puct_round_kernel's and gz_puct_reroot's one-node roots), and not in
// a kernel of its own: roots appear in any round of gz_selfplay_puct_rounds, so a
// separate kernel would be one more launch in every round, while here a round without
// a new root pays one uniform branch.
__global__ __launch_bounds__(WAVE) void puct_backup_kernel(char* ws, int n, int S, const double* prior,
                                                           const float* value, PuctNoise nz) {
    const int g = blockIdx.x;
    if (g >= n) return;
    const int lane = lane_id();
    PuctTree t = tree_of(ws, g, S);
    const int j = t.h->pending;
    if (j < 0) return;
    for (int c = lane; c < GZ_CELLS; c += WAVE) t.prior[(size_t)j * GZ_CELLS + c] = prior[(size_t)g * GZ_CELLS + c];
    if (j == 0 && t.h->full) {  // (a fast ply's root keeps the evaluator's row)
        const PuctNoise z = noise_of(nz, ws);
        if (z.on) mix_root_row(t, z);  // (each lane mixes the cells it has just stored)
    }
    if (lane == 0) {
        const float v = value[g];
        t.value[j] = v;
        backup(t, j, (double)v);
        t.h->pending = -1;
        t.h->n_evals += 1;
        t.h->new_evals += 1;
    }
}

// ---------------------------------------------------------------- leaf batching
// Between two descents of one launch: every store of the wave (lane 0's tree words, the
// node rows of all lanes, vl in LDS) has left and is visible to every lane before the
// next descent's first load.  The wave is alone in its workgroup, so workgroup scope is
// the whole audience.
__device__ inline void batch_sync() {
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __syncthreads();
}

// Up to K descents of game g's tree, one after the other (each sees the virtual losses
// of those before it); the semantics are in the header comment.  vl: int16 [S+1], LDS.
__global__ __launch_bounds__(WAVE) void puct_select_batch_kernel(char* ws, int n, int S, int K, int16_t* pend,
                                                                 uint32_t* leaves, int32_t* active) {
    extern __shared__ __attribute__((aligned(16))) int16_t vl[];
    const int g = blockIdx.x;
    if (g >= n) return;
    const int lane = lane_id();
    const double c_puct = ((const PuctCfg*)ws)->c_puct;
    const PuctTree t = tree_of(ws, g, S);
    PuctHdr* h = t.h;
    int16_t* pd = pend + (size_t)g * K;
    for (int x = lane; x <= S; x += WAVE) vl[x] = 0;
    BB rblack, rwhite;
    load_bb(rblack, h->black);
    load_bb(rwhite, h->white);
    const int player0 = h->player, cnt0 = h->n_moves;
    const int first = h->n_nodes;  // nodes from here on are created in this launch
    // (pending: the root still waits for its backup; keep the tree as it is)
    bool go = !(h->over || h->pending >= 0);
    int k = 0;
    batch_sync();
    while (go && k < K) {
        if (t.visits[0] + vl[0] > S) break;  // finished + in-flight simulations fill the budget
        BB black = rblack, white = rwhite;
        int mover = player0, cnt = cnt0;
        int i = 0;
        while (true) {
            const int tm = t.term[i];
            if (tm) {
                if (lane == 0) backup(t, i, tm == 3 ? 0.0 : -1.0);
                break;
            }
            const BB E = empties(black, white);
            const double sq = __builtin_sqrt((double)(t.visits[i] + vl[i]));
            const double* pr = t.prior + (size_t)i * GZ_CELLS;
            const int16_t* ch = t.child + (size_t)i * GZ_CELLS;
            double bv = -__builtin_inf();
            int bi = INT_MAX;
#pragma unroll
            for (int q4 = 0; q4 < 4; q4++) {
                const int c = lane + WAVE * q4;
                if (c < GZ_CELLS && bb_test(E, cell_to_bit(c))) {
                    const int cj = ch[c];
                    int nn = 0;
                    double q = 0.0;
                    if (cj >= 0) {
                        const int lost = vl[cj];
                        nn = t.visits[cj] + lost;
                        q = nn ? (t.W[cj] - (double)lost) / (double)nn : 0.0;
                    }
                    const double u = ((c_puct * pr[c]) * sq) / (1.0 + (double)nn);
                    const double sc = q + u;
                    if (sc > bv) {
                        bv = sc;
                        bi = c;
                    }
                }
            }
            wave_argmax(bv, bi);
            if (bi == INT_MAX) bi = bit_to_cell(lowest_bit(E));  // only if the evaluator gave non-finite priors
            if (bi < 0 || bi >= GZ_CELLS) {  // (a live node always has an empty cell)
                go = false;
                break;
            }
            const int bit = cell_to_bit(bi);
            const int cj = ch[bi];
            if (cj >= 0) {
                if (cj >= first && t.term[cj] == 0) {  // a collision: the node has no prior row yet
                    go = false;
                    break;
                }
                if (mover == 1) bb_set(black, bit);
                else bb_set(white, bit);
                mover = 3 - mover;
                cnt++;
                i = cj;
                continue;
            }
            const int j = h->n_nodes;
            if (j > S) {  // (never within the budget: every descent creates at most one node)
                go = false;
                break;
            }
            // make_move's rules, as descend()
            const bool win = bb_test(threats(mover == 1 ? black : white).win, bit);
            const int ne = bb_count(E);
            if (mover == 1) bb_set(black, bit);
            else bb_set(white, bit);
            cnt++;
            const int term = win ? mover : ((ne == 1 || cnt >= GZ_MAX_GAME_PLIES) ? 3 : 0);
            new_node(t, j, i, bi, term, black, white, term != 0);
            if (lane == 0) {
                t.child[(size_t)i * GZ_CELLS + bi] = (int16_t)j;
                h->n_nodes = j + 1;
                if (term) {
                    backup(t, j, term == 3 ? 0.0 : -1.0);
                } else {
                    pd[k] = (int16_t)j;
                    vl[j] += 1;
                    for (int x = i; x >= 0; x = t.parent[x]) vl[x] += 1;
                }
            }
            if (term == 0) {
                write_leaf(leaves, active, g * K + k, black, white, true);
                k++;
            }
            break;
        }
        batch_sync();
    }
    for (; k < K; k++) {
        write_leaf(leaves, active, g * K + k, rblack, rwhite, false);
        if (lane == 0) pd[k] = -1;
    }
}

// The backup step of a batched round: the root of gz_puct_begin (header.pending, row g K,
// with the root-noise branch of puct_backup_kernel), else the game's active rows in
// ascending order -- the prior rows by the whole wave, values and backups by lane 0 one
// row after the other, so every W sums in the reference's order.
__global__ __launch_bounds__(WAVE) void puct_backup_batch_kernel(char* ws, int n, int S, int K, int16_t* pend,
                                                                 const double* prior, const float* value,
                                                                 PuctNoise nz) {
    const int g = blockIdx.x;
    if (g >= n) return;
    const int lane = lane_id();
    PuctTree t = tree_of(ws, g, S);
    PuctHdr* h = t.h;
    const int j0 = h->pending;
    if (j0 >= 0) {
        const size_t row = (size_t)g * K;
        for (int c = lane; c < GZ_CELLS; c += WAVE) t.prior[(size_t)j0 * GZ_CELLS + c] = prior[row * GZ_CELLS + c];
        if (j0 == 0 && h->full) {
            const PuctNoise z = noise_of(nz, ws);
            if (z.on) mix_root_row(t, z);  // (each lane mixes the cells it has just stored)
        }
        if (lane == 0) {
            const float v = value[row];
            t.value[j0] = v;
            backup(t, j0, (double)v);
            h->pending = -1;
            h->n_evals += 1;
            h->new_evals += 1;
        }
        return;
    }
    int16_t* pd = pend + (size_t)g * K;
    for (int k = 0; k < K; k++) {
        const int j = pd[k];
        if (j < 0 || j > S) continue;
        const size_t row = (size_t)g * K + k;
        for (int c = lane; c < GZ_CELLS; c += WAVE) t.prior[(size_t)j * GZ_CELLS + c] = prior[row * GZ_CELLS + c];
        if (lane == 0) {
            const float v = value[row];
            t.value[j] = v;
            backup(t, j, (double)v);
            h->n_evals += 1;
            h->new_evals += 1;
        }
    }
    // every lane has read the game's pend row before it is cleared
    batch_sync();
    for (int k = lane; k < K; k += WAVE) pd[k] = -1;
}

// simulations left to every game's budget (0: the game is over), and their maximum
__global__ void puct_remaining_kernel(char* ws, int n, int S, int32_t* remaining, int32_t* largest) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    const PuctTree t = tree_of(ws, g, S);
    int r = t.h->over ? 0 : t.h->budget + 1 - t.visits[0];
    if (r < 0) r = 0;
    if (remaining) remaining[g] = r;
    if (largest && r > 0) atomicMax(largest, r);
}

// ---------------------------------------------------------------- finish
// the root-child visit counts of this lane's cells (v[k]: cell lane + 64 k); returns their sum
__device__ inline long long root_visits(const PuctTree& t, bool over, int v[4]) {
    const int lane = lane_id();
    long long tot = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = lane + WAVE * k;
        v[k] = 0;
        if (c < GZ_CELLS) {
            const int cj = over ? -1 : t.child[c];
            if (cj >= 0) v[k] = t.visits[cj];
        }
        tot += v[k];
    }
    return wave_sum_ll(tot);
}

// the move of a live root from its visit counts (root_visits); draws: main-stream draws used
__device__ inline int pick_move(const PuctHdr* h, const PuctCfg& cfg, const BB& E, const int v[4], long long total,
                                int& draws) {
    const int lane = lane_id();
    int mv = -1;
    draws = 0;
    if (h->n_moves >= cfg.temp_plies || total == 0) {
        // most visits, first maximum (occupied cells never win: -1)
        int bv = -2, bi = INT_MAX;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = lane + WAVE * k;
            if (c < GZ_CELLS) {
                const int x = bb_test(E, cell_to_bit(c)) ? v[k] : -1;
                if (x > bv) {
                    bv = x;
                    bi = c;
                }
            }
        }
        wave_argmax_int(bv, bi);
        mv = bi;
    } else {
        // one draw of the game's main stream; the first cell whose running visit
        // sum exceeds pick = (draw * total) >> 64
        const uint64_t key = stream_key(cfg.seed, h->game_id, h->n_moves, 0);
        const uint64_t pick = __umul64hi(draw(key, 0), (uint64_t)total);
        draws = 1;
        long long base = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            long long inc = v[k];
#pragma unroll
            for (int off = 1; off < WAVE; off <<= 1) {
                const long long o = __shfl_up(inc, off);
                if (lane >= off) inc += o;
            }
            const uint64_t hit = ballot((uint64_t)(base + inc) > pick);
            if (mv < 0 && hit) mv = WAVE * k + (int)__builtin_ctzll(hit);
            base += __shfl(inc, WAVE - 1);
        }
    }
    return mv;
}

__device__ inline gz_search_stats search_stats(int n_nodes, int predicts, int draws, long long sim_draws) {
    gz_search_stats st;
    st.n_nodes = n_nodes;
    st.predicts = predicts;
    st.main_draws = draws;
    st.pad = 0;
    st.sim_draws = sim_draws;
    return st;
}

__global__ __launch_bounds__(WAVE) void puct_finish_kernel(char* ws, int n, int S, int32_t* moves, int32_t* visits,
                                                           double* root_q, gz_search_stats* stats) {
    const int g = blockIdx.x;
    if (g >= n) return;
    const int lane = lane_id();
    const PuctCfg cfg = *(const PuctCfg*)ws;
    PuctTree t = tree_of(ws, g, S);
    PuctHdr* h = t.h;
    BB black, white;
    load_bb(black, h->black);
    load_bb(white, h->white);
    const BB E = empties(black, white);
    const bool over = h->over != 0;
    int v[4];
    const long long total = root_visits(t, over, v);
    if (visits) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (lane + WAVE * k < GZ_CELLS) visits[(size_t)g * GZ_CELLS + lane + WAVE * k] = v[k];
    }
    int mv = -1, draws = 0;
    if (!over) mv = pick_move(h, cfg, E, v, total, draws);
    if (lane == 0) {
        moves[g] = mv;
        // the root's mean value for the side to move (W[0] is the opponent's view)
        if (root_q) root_q[g] = (over || t.visits[0] == 0) ? 0.0 : -t.W[0] / (double)t.visits[0];
        h->move = mv;
        h->main_draws = draws;
        if (stats) stats[g] = search_stats(over ? 0 : h->n_nodes, h->n_evals, draws, 0);
    }
}

// ---------------------------------------------------------------- tree reuse
// Re-root game t at its node c (1 <= c < n_nodes): the subtree of c becomes the tree, the
// header's position advances by c's move.  The whole workgroup (RR_THREADS; every thread
// calls) works on the one game; map [S+1], list [S+1]: LDS.
//   mark    wave 0: keep[j] = j == c || keep[parent[j]], 64 nodes at a time in ascending
//           order (parents precede children; inside a chunk the flags are propagated
//           until they stand), new index = rank among the kept: map[old] = new or -1,
//           list[new] = old;
//   move    every array's kept rows to their new places in ascending order.  new < old
//           for every kept node, so a batch reads [U x RR_THREADS elements at or above
//           their old places], waits for them (every wave, then a barrier), then writes
//           places below everything still to be read: in place, no second tree.
constexpr int RR_THREADS = 1024;

template <typename T, int W, int U, typename F>
__device__ inline void move_rows(T* a, const int16_t* list, int kept, F f) {
    const int tid = threadIdx.x;
    const int total = kept * W;
    for (int i0 = 0; i0 < total; i0 += U * RR_THREADS) {
        T v[U] = {};
#pragma unroll
        for (int k = 0; k < U; k++) {
            const int idx = i0 + k * RR_THREADS + tid;
            if (idx < total) {
                const int nj = idx / W;
                v[k] = a[(size_t)list[nj] * W + (idx - nj * W)];
            }
        }
        // every load of the batch has returned before its first store leaves
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
#pragma unroll
        for (int k = 0; k < U; k++) {
            const int idx = i0 + k * RR_THREADS + tid;
            if (idx < total) a[idx] = f(v[k]);
        }
    }
}

__device__ inline void reroot(const PuctTree& t, int c, int S, int16_t* map, int16_t* list) {
    __shared__ int info[2];  // kept nodes, evaluated ones among them
    const int tid = threadIdx.x, lane = lane_id();
    PuctHdr* h = t.h;
    const int n = h->n_nodes < S + 1 ? h->n_nodes : S + 1;
    const int pend = h->pending;
    if (tid < WAVE) {
        int kept = 0, evals = 0;
        for (int base = 0; base < n; base += WAVE) {
            const int j = base + lane;
            const bool in = j < n;
            const int p = in ? t.parent[j] : -1;
            const int sh = p >= base ? p - base : 0;  // the parent's lane when it is in this chunk
            bool k = in && (j == c || (p >= 0 && p < base && map[p] >= 0));
            uint64_t m = ballot(k);
            while (true) {
                k = k || (in && p >= base && ((m >> sh) & 1));
                const uint64_t nm = ballot(k);
                if (nm == m) break;
                m = nm;
            }
            const int nj = kept + rank_in(m);
            if (in) map[j] = k ? (int16_t)nj : (int16_t)-1;
            if (k) list[nj] = (int16_t)j;
            evals += __popcll(ballot(k && j != pend && t.term[j] == 0));
            kept += __popcll(m);
            __threadfence_block();  // this wave's map is written before the next chunk reads it
        }
        if (lane == 0) {
            info[0] = kept;
            info[1] = evals;
        }
    }
    __syncthreads();
    const int kept = info[0], evals = info[1];
    for (int nb = 0; nb < kept; nb += RR_THREADS) {  // the scalars, one node per thread
        const int nj = nb + tid;
        const bool in = nj < kept;
        double w = 0.0;
        float va = 0.0f;
        int vi = 0, pa = 0;
        uint8_t mo = 0, te = 0;
        if (in) {
            const int j = list[nj];
            w = t.W[j];
            vi = t.visits[j];
            va = t.value[j];
            pa = t.parent[j];
            mo = t.move[j];
            te = t.term[j];
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (in) {
            t.W[nj] = w;
            t.visits[nj] = vi;
            t.value[nj] = va;
            t.parent[nj] = nj == 0 ? (int16_t)-1 : map[pa];
            t.move[nj] = nj == 0 ? (uint8_t)255 : mo;
            t.term[nj] = te;
        }
    }
    move_rows<uint32_t, 16, 4>(t.board, list, kept, [](uint32_t x) { return x; });
    move_rows<double, GZ_CELLS, 8>(t.prior, list, kept, [](double x) { return x; });
    move_rows<int16_t, GZ_CELLS, 8>(t.child, list, kept,
                                    [map](int16_t x) { return x >= 0 ? map[x] : (int16_t)-1; });
    __syncthreads();
    if (tid < 16) ((uint32_t*)h)[tid] = t.board[tid];  // black[8], white[8]: the new root's board
    if (tid == 0) {
        h->n_moves += 1;
        h->player = 3 - h->player;
        h->over = t.term[0] != 0;
        h->n_nodes = kept;
        h->n_evals = evals;
        h->main_draws = 0;
        h->pending = pend >= 0 ? map[pend] : -1;
        h->move = -1;
    }
    __syncthreads();
}

// gz_puct_reroot: the step API's move between two searches
__global__ __launch_bounds__(RR_THREADS) void puct_reroot_kernel(char* ws, int n, int S, const int32_t* moves,
                                                                 uint32_t* leaves, int32_t* active,
                                                                 int32_t* remaining) {
    extern __shared__ __attribute__((aligned(16))) int16_t remap[];
    const int g = blockIdx.x;
    if (g >= n) return;
    PuctTree t = tree_of(ws, g, S);
    PuctHdr* h = t.h;
    BB black, white;
    load_bb(black, h->black);
    load_bb(white, h->white);
    const BB E = empties(black, white);
    const int m = moves[g];
    const bool play = m >= 0 && m < GZ_CELLS && !h->over && bb_test(E, cell_to_bit(m));
    int c = play ? t.child[m] : -1;
    if (c >= h->n_nodes) c = -1;
    __syncthreads();  // (every thread has read the header before any of it changes)
    if (c > 0) reroot(t, c, S, remap, remap + S + 1);
    if (threadIdx.x >= WAVE) return;
    PuctCap cap = {};
    cap.on = -1;  // as gz_puct_begin stored it
    cap = cap_of(cap, ws);
    const uint64_t seed = ((const PuctCfg*)ws)->seed;
    // an inherited root: the budget of its new ply; when live and full, its carried row is
    // mixed once, with the key of that ply (a root that still waits for its evaluation is
    // mixed at that backup)
    if (c > 0) {
        const bool full = set_budget(h, cap, seed, S);
        if (full && !h->over && h->pending != 0) {
            PuctNoise stored = {};
            stored.on = -1;
            const PuctNoise nz = noise_of(stored, ws);
            if (nz.on) mix_root_row(t, nz);
        }
    }
    bool live = false;
    if (play && c <= 0) {
        // no node under the move: a fresh root that waits for its evaluation
        const int bit = cell_to_bit(m), mover = h->player, cnt = h->n_moves + 1;
        const bool win = bb_test(threats(mover == 1 ? black : white).win, bit);
        const bool over = win || bb_count(E) == 1 || cnt >= GZ_MAX_GAME_PLIES;
        if (mover == 1) bb_set(black, bit);
        else bb_set(white, bit);
        const int64_t gid = h->game_id;
        const int32_t reuse = h->reuse;
        const bool full = root_is_full(cap, seed, gid, cnt);
        begin_root(t, black, white, gid, cnt, 3 - mover, over, reuse, full ? S : cap.fast, full);
        live = !over;
        __threadfence_block();
    }
    write_leaf(leaves, active, g, black, white, live);
    if (remaining && threadIdx.x == 0) {
        const int r = h->over ? 0 : h->budget + 1 - t.visits[0];  // (thread 0 wrote the budget itself)
        remaining[g] = r < 0 ? 0 : r;
    }
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

// Round step 1: a slot whose search is at its budget (B + 1 root visits or more) picks
// its move (wave 0), stashes the visit row of the ply and hands move and statistics to
// selfplay_commit_kernel
// (move -1 leaves the slot alone); then the workgroup re-roots the tree under the move,
// unless the move ends the game -- the tree of a move that ends it no longer matches
// its slot after the commit, and puct_round_kernel begins a fresh one.
__global__ __launch_bounds__(RR_THREADS) void puct_advance_kernel(const char* slots, int n, gz_puct_params p,
                                                                  PuctNoise nz, PuctCap cap, char* ws, int32_t* moves,
                                                                  gz_search_stats* stats, uint16_t* pend) {
    extern __shared__ __attribute__((aligned(16))) int16_t remap[];
    __shared__ int next_root;
    const int s = blockIdx.x;
    if (s >= n) return;
    const int S = p.num_simulations;
    PuctTree t = tree_of(ws, s, S);
    PuctHdr* h = t.h;
    if (threadIdx.x < WAVE) {
        const int lane = lane_id();
        const SlotHeader* sh = slot_of(slots, s);
        const bool due = sh->game_id < sh->game_id_end && tree_matches(h, sh) && !h->over && h->pending < 0 &&
                         t.visits[0] >= h->budget + 1 && h->n_moves >= 0 && h->n_moves < GZ_MAX_GAME_PLIES;
        int mv = -1, c = -1;
        if (due) {
            PuctCfg cfg;
            cfg.c_puct = p.c_puct;
            cfg.seed = p.seed;
            cfg.temp_plies = p.temp_plies;
            cfg.S = S;
            BB black, white;
            load_bb(black, h->black);
            load_bb(white, h->white);
            int v[4], draws;
            const long long total = root_visits(t, false, v);
            mv = pick_move(h, cfg, empties(black, white), v, total, draws);
            uint16_t* row = pend + ((size_t)s * GZ_MAX_GAME_PLIES + h->n_moves) * GZ_CELLS;
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (lane + WAVE * k < GZ_CELLS) row[lane + WAVE * k] = (uint16_t)v[k];
            if (mv >= 0 && mv < GZ_CELLS) {
                c = t.child[mv];
                if (c <= 0 || c >= h->n_nodes || c > S || t.term[c]) c = -1;
            }
            if (lane == 0) {
                // (the third statistic, RNG draws of the simulations elsewhere: the rounds the move took)
                stats[s] = search_stats(h->n_nodes, h->new_evals, draws, h->rounds);
                h->move = mv;
                h->main_draws = draws;
                h->new_evals = 0;
                h->rounds = 0;
            }
        }
        if (lane == 0) {
            moves[s] = mv;
            next_root = c;
        }
    }
    __syncthreads();
    if (next_root > 0) {
        reroot(t, next_root, S, remap, remap + S + 1);
        // the inherited root (live, evaluated): its new ply's budget and, on a full ply, its
        // carried row mixed with that ply's key
        if (threadIdx.x < WAVE) {
            const bool full = set_budget(h, cap, p.seed, S);
            if (nz.on && full) mix_root_row(t, nz);
        }
    }
}

// Round step 3: a tree that is not the slot's (a new game, a reset, a move that ended
// the game) gives way to a fresh root, whose board is its leaf of this round; every
// other slot descends once.
__global__ __launch_bounds__(WAVE) void puct_round_kernel(const char* slots, int n, gz_puct_params p, PuctCap cap,
                                                          char* ws, uint32_t* leaves, int32_t* active) {
    const int s = blockIdx.x;
    if (s >= n) return;
    const int S = p.num_simulations;
    const SlotHeader* sh = slot_of(slots, s);
    PuctTree t = tree_of(ws, s, S);
    PuctHdr* h = t.h;
    BB black, white;
    load_bb(black, sh->black);
    load_bb(white, sh->white);
    if (sh->game_id >= sh->game_id_end) {  // idle: its games are done
        write_leaf(leaves, active, s, black, white, false);
        return;
    }
    const int rounds = h->reuse == REUSE_MAGIC ? h->rounds : 0;
    if (tree_matches(h, sh)) {
        descend(t, p.c_puct, S, s, leaves, active);
    } else {
        const bool full = root_is_full(cap, p.seed, sh->game_id, sh->n_moves);
        begin_root(t, black, white, sh->game_id, sh->n_moves, sh->player, false, REUSE_MAGIC, full ? S : cap.fast,
                   full);
        write_leaf(leaves, active, s, black, white, true);
    }
    if (lane_id() == 0) h->rounds = rounds + 1;
}

__global__ void puct_reset_kernel(char* ws, int n, int S) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    PuctHdr* h = tree_of(ws, g, S).h;
    h->reuse = 0;
    h->n_nodes = 0;
    h->pending = -1;
    h->move = -1;
}

// ---------------------------------------------------------------- export
__global__ __launch_bounds__(256) void puct_export_kernel(const char* ws, int n, int S, char* out) {
    const int g = blockIdx.x;
    if (g >= n) return;
    const size_t M = (size_t)S + 1;
    const char* src = ws + 256 + (size_t)g * game_stride_for(S);
    char* dst = out + (size_t)g * export_bytes_for(S);
    const PuctHdr* h = (const PuctHdr*)src;
    if (threadIdx.x == 0) {
        int32_t* o = (int32_t*)dst;
        o[0] = h->n_nodes;
        o[1] = h->n_evals;
        o[2] = h->main_draws;
        o[3] = h->move;
    }
    // W .. board: 1880 M bytes, 4-byte words on both sides
    const uint32_t* a = (const uint32_t*)(src + sizeof(PuctHdr));
    uint32_t* b = (uint32_t*)(dst + 16);
    for (size_t w = threadIdx.x; w < 470 * M; w += 256) b[w] = a[w];
    // parent, move, term: 4 M bytes after the child table
    const char* c = src + sizeof(PuctHdr) + 2330 * M;
    char* d = dst + 16 + 1880 * M;
    for (size_t w = threadIdx.x; w < 4 * M; w += 256) d[w] = c[w];
}

// int32 visit row of the search -> the slot's pending uint16 row of this ply
__global__ __launch_bounds__(WAVE) void puct_stash_kernel(const gz_board_state* boards, const int32_t* moves,
                                                          const int32_t* visits, int n, uint16_t* pend) {
    const int s = blockIdx.x;
    if (s >= n) return;
    const int ply = boards[s].n_moves;
    if (moves[s] < 0 || ply < 0 || ply >= GZ_MAX_GAME_PLIES) return;
    uint16_t* row = pend + ((size_t)s * GZ_MAX_GAME_PLIES + ply) * GZ_CELLS;
    for (int c = lane_id(); c < GZ_CELLS; c += WAVE) row[c] = (uint16_t)visits[(size_t)s * GZ_CELLS + c];
}

// gz_puct_root_noise: eta of every board's root (ply = n_moves), root_eta as the search runs it
__global__ __launch_bounds__(WAVE) void puct_root_noise_kernel(const gz_board_state* boards, const int64_t* game_ids,
                                                               int n, uint64_t seed, double alpha, double* out) {
    const int g = blockIdx.x;
    if (g >= n) return;
    const int lane = lane_id();
    BB black, white;
    load_bb(black, boards[g].black);
    load_bb(white, boards[g].white);
    double eta[4];
    root_eta(empties(black, white), seed, game_ids[g], boards[g].n_moves, alpha, eta);
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (lane + WAVE * k < GZ_CELLS) out[(size_t)g * GZ_CELLS + lane + WAVE * k] = eta[k];
}

// gz_puct_cap_full: one thread per record, the decision of its (game id, ply)
__global__ __launch_bounds__(256) void puct_cap_full_kernel(const gz_record* records, int n, uint64_t seed,
                                                            double full_prob, uint8_t* out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = cap_is_full(seed, records[i].game_id, records[i].ply, full_prob) ? 1 : 0;
}

// ---------------------------------------------------------------- slot compaction
// gz_selfplay_puct_compact (the header comment has the scheme).  The plan in the
// workspace: int32 n_pairs (16 bytes), holes [cap], fillers [cap].
constexpr int CP_THREADS = 256;
constexpr int CP_PARTS = 8;  // workgroups that share the bytes of one pair

// One workgroup scans the first n slots in tiles of 1024 (the ballot and prefix scheme of
// selfplay_order_kernel): pass 0 counts the active slots, a; pass 1 ranks the holes (idle,
// index < a) and the fillers (active, index >= a), each ascending; then the k-th filler is
// paired with the k-th hole.  order[s] = s except at the pairs, which trade places.
__global__ __launch_bounds__(1024) void puct_compact_plan_kernel(const char* slots, int n, int cap, int32_t* order,
                                                                 int32_t* n_active, int32_t* plan) {
    __shared__ int wsum[2][16];
    __shared__ int carry[2], total;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
            if (pass == 1) {
                if (x) holes[bx + __popcll(mx & below)] = s;
                if (y) fillers[by + __popcll(my & below)] = s;
                if (in && !x && !y) order[s] = s;
            }
            __syncthreads();
            if (tid == 0) {
                for (int w = 0; w < 16; w++) {
                    carry[0] += wsum[0][w];
                    carry[1] += wsum[1][w];
                }
            }
            __syncthreads();
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
    // W, prior, visits, value, board, child, parent, move, term: bytes per node, as tree_of
    const int width[9] = {8, 1800, 4, 4, 64, 450, 2, 1, 1};
    size_t off = sizeof(PuctHdr);
#pragma unroll
    for (int a = 0; a < 9; a++) {
        copy_span(dst + off, src + off, (size_t)width[a] * nn, part);
        off += width[a] * M;
    }
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

// ---------------------------------------------------------------- the match (two networks)
// gz_puct_match_run (the header comment has the scheme).  Side A is index 0, B index 1;
// A plays black in game g iff ((g ^ parity) & 1) == 0, and the mover's side evaluates
// every leaf of its search.
__device__ inline int match_side(int64_t game_id, int player, int parity) {
    const bool a_black = (((int)(game_id & 1) ^ parity) & 1) == 0;
    return (player == 1) == a_black ? 0 : 1;
}

// Once per ply, one workgroup over the first n slots in tiles of 1024 (the ballot and
// prefix scheme of puct_compact_plan_kernel): side[s] = the mover's side or -1 for an idle
// slot, row_of[s] = the slot's rank among the slots of its side in ascending slot order,
// count[0..1] = the slots per side.  An idle slot's board is marked over, so the search
// leaves it alone (no leaf, no backup, move -1) whatever its prior and value rows hold.
__global__ __launch_bounds__(1024) void puct_match_plan_kernel(const char* slots, int n, int parity,
                                                               gz_board_state* boards, int32_t* side,
                                                               int32_t* row_of, int32_t* count) {
    __shared__ int wsum[2][16];
    __shared__ int carry[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
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
        const uint64_t m0 = __ballot(sd == 0), m1 = __ballot(sd == 1);
        if (lane == 0) {
            wsum[0][wave] = __popcll(m0);
            wsum[1][wave] = __popcll(m1);
        }
        __syncthreads();
        int b0 = carry[0], b1 = carry[1];
        for (int w = 0; w < wave; w++) {
            b0 += wsum[0][w];
            b1 += wsum[1][w];
        }
        const uint64_t below = (1ull << lane) - 1;
        if (s < n) {
            side[s] = sd;
            row_of[s] = sd == 0 ? b0 + __popcll(m0 & below) : (sd == 1 ? b1 + __popcll(m1 & below) : 0);
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 0; w < 16; w++) {
                carry[0] += wsum[0][w];
                carry[1] += wsum[1][w];
            }
        }
        __syncthreads();
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

inline hipStream_t as_stream(void* s) { return (hipStream_t)s; }

int check_alpha(const char* who, double alpha) {
    if (!(alpha >= 1e-3 && alpha <= 1e3))  // (a NaN fails both)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": noise alpha must be finite and in [1e-3, 1e3]");
    return GZ_OK;
}

// The root noise p asks for.  Only with GZ_PUCT_ROOT_NOISE set is p a
// gz_puct_noise_params; without it nothing past the 32 bytes of gz_puct_params is read.
int read_noise(const char* who, const gz_puct_params* p, PuctNoise& nz) {
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

// The leaves per round p asks for: 0 without GZ_PUCT_LEAF_BATCH (nothing past the noise
// struct is read then), else gz_puct_batch_params.leaves_per_round in 1..GZ_PUCT_MAX_LEAVES.
int read_leaves(const char* who, const gz_puct_params* p, int& K) {
    K = 0;
    if (!(p->flags & GZ_PUCT_LEAF_BATCH)) return GZ_OK;
    K = ((const gz_puct_batch_params*)p)->leaves_per_round;
    if (K < 1 || K > GZ_PUCT_MAX_LEAVES)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": leaves_per_round out of range [1, 32]");
    return GZ_OK;
}

int check_full_prob(const char* who, double full_prob) {
    if (!(full_prob >= 0.0 && full_prob <= 1.0))  // (a NaN fails both)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": full_prob must be finite and in [0, 1]");
    return GZ_OK;
}

// The playout cap p asks for.  Only with GZ_PUCT_PLAYOUT_CAP set is p a gz_puct_cap_params;
// without it nothing past the batch struct is read.  (After check_S: F is held against S.)
int read_cap(const char* who, const gz_puct_params* p, PuctCap& cap) {
    cap.full_prob = 1.0;
    cap.fast = p->num_simulations;
    cap.on = 0;
    if (!(p->flags & GZ_PUCT_PLAYOUT_CAP)) return GZ_OK;
    if (p->flags & GZ_PUCT_LEAF_BATCH)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": the playout cap with leaf batching is not supported");
    const gz_puct_cap_params* q = (const gz_puct_cap_params*)p;
    if (q->fast_simulations < 1 || q->fast_simulations > p->num_simulations)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": fast_simulations out of range [1, num_simulations]");
    int rc = check_full_prob(who, q->full_prob);
    if (rc) return rc;
    cap.full_prob = q->full_prob;
    cap.fast = q->fast_simulations;
    cap.on = 1;
    return GZ_OK;
}

// the n K rows of a round are indexed with int32
int check_rows(const char* who, int32_t n, int32_t K) {
    if (K > 0 && (int64_t)n * K > INT32_MAX) return gz_fail(GZ_ERR_ARG, std::string(who) + ": n x leaves_per_round too large");
    return GZ_OK;
}

// Which workspaces hold a batched search.  gz_puct_select, gz_puct_backup and
// gz_puct_reroot take no params, and the kernel to launch (and its grid of rows) cannot
// be chosen from the PuctCfg in device memory without reading it back, which would
// synchronise the unbatched step API too.  So gz_puct_begin notes K on the host as well,
// by workspace address; a later unbatched begin on the same address removes the note.
std::mutex g_batch_mutex;
std::unordered_map<const void*, int> g_batch_leaves;

void note_leaves(const void* ws, int K) {
    std::lock_guard<std::mutex> lock(g_batch_mutex);
    if (K > 0) g_batch_leaves[ws] = K;
    else if (!g_batch_leaves.empty()) g_batch_leaves.erase(ws);
}

int leaves_of(const void* ws) {
    std::lock_guard<std::mutex> lock(g_batch_mutex);
    if (g_batch_leaves.empty()) return 0;
    const auto it = g_batch_leaves.find(ws);
    return it == g_batch_leaves.end() ? 0 : it->second;
}

int backup_impl(void* ws, int32_t n, int32_t S, const double* d_prior, const float* d_value, const PuctNoise& nz,
                void* stream) {
    puct_backup_kernel<<<n, WAVE, 0, as_stream(stream)>>>((char*)ws, n, S, d_prior, d_value, nz);
    return gz_check_launch("puct_backup_kernel");
}

// GZ_PUCT_LEAF_SYM (gz_sym.h, gz_pvsym.hip): t is the extra region behind the flag-clear
// workspace, one byte per row of the round buffers; nullptr with the flag clear, and then
// neither step launches anything.  sym_leaves turns the round's leaf rows in place -- the
// select, begin and round kernels rewrite every row of every round and nothing but the
// forward reads the buffer (the backup kernels take no leaf pointer; a node's board is in
// its tree) -- and sym_priors maps the forward's prior rows back before the backup, which
// reads nothing else of the 225-wide buffers.
struct LeafSym {
    uint8_t* t;
    uint64_t seed;
};

LeafSym leaf_sym(const gz_puct_params* p, void* ws, size_t flag_clear_bytes) {
    LeafSym ls;
    ls.t = (p->flags & GZ_PUCT_LEAF_SYM) ? (uint8_t*)ws + flag_clear_bytes : nullptr;
    ls.seed = p->seed;
    return ls;
}

int sym_leaves(const LeafSym& ls, uint32_t* leaves, int32_t rows, void* stream) {
    if (!ls.t) return GZ_OK;
    return gz_internal_sym_boards(leaves, leaves, rows, nullptr, nullptr, ls.seed, ls.t, stream);
}

int sym_priors(const LeafSym& ls, double* prior, int32_t rows, void* stream) {
    if (!ls.t) return GZ_OK;
    return gz_internal_sym_rows(nullptr, nullptr, prior, rows, nullptr, ls.t, stream);
}

struct RoundBufs {
    uint32_t* leaves;
    int32_t* active;
    float *logits, *probs, *value;
    double* prior;
    void* pvws;
};

// reroot()'s LDS: map and list, int16 [S+1] each
size_t remap_bytes(int32_t S) { return (4 * ((size_t)S + 1) + 15) & ~(size_t)15; }

size_t rounds_offset(int32_t n, int32_t S) { return 256 + (size_t)n * game_stride_for(S); }

// the round buffers of n rows from p on
RoundBufs carve_rows(char* p, size_t n) {
    RoundBufs r;
    r.leaves = (uint32_t*)p;
    p += al256((size_t)n * 64);
    r.active = (int32_t*)p;
    p += al256((size_t)n * 4);
    r.logits = (float*)p;
    p += al256((size_t)n * 900);
    r.probs = (float*)p;
    p += al256((size_t)n * 900);
    r.value = (float*)p;
    p += al256((size_t)n * 4);
    r.prior = (double*)p;
    p += al256((size_t)n * 1800);
    r.pvws = p;
    return r;
}

// (n: the game count the workspace was sized for -- a search of fewer games on it finds
// every buffer where the full one does)
RoundBufs carve_rounds(void* ws, int32_t n, int32_t S) { return carve_rows((char*)ws + rounds_offset(n, S), n); }

// the batched workspace after the trees: pend i16 [n][K], the remaining count, then the
// round buffers of n K rows
struct BatchBufs {
    int16_t* pend;
    int32_t* left;
    RoundBufs r;
};

size_t batch_pend_bytes(int32_t n, int32_t K) { return al256((size_t)n * K * 2); }

BatchBufs carve_batch(void* ws, int32_t n, int32_t S, int32_t K) {
    char* p = (char*)ws + rounds_offset(n, S);
    BatchBufs b;
    b.pend = (int16_t*)p;
    p += batch_pend_bytes(n, K);
    b.left = (int32_t*)p;
    p += 256;
    b.r = carve_rows(p, (size_t)n * K);
    return b;
}

int check_S(const char* who, int32_t n, int32_t S) {
    if (S < 1 || S > GZ_MAX_SIMULATIONS)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": num_simulations out of range [1, 4095]");
    if (n < 0) return gz_fail(GZ_ERR_ARG, std::string(who) + ": n < 0");
    return GZ_OK;
}

int finish_impl(void* ws, int32_t n, int32_t S, int32_t* d_moves, int32_t* d_visits, double* d_root_q,
                gz_search_stats* d_stats, void* stream) {
    puct_finish_kernel<<<n, WAVE, 0, as_stream(stream)>>>((char*)ws, n, S, d_moves, d_visits, d_root_q, d_stats);
    return gz_check_launch("puct_finish_kernel");
}

// n_cap: the game count that carved the workspace (the place of pend), n <= n_cap games run
int select_batch_impl(void* ws, int32_t n_cap, int32_t n, int32_t S, int32_t K, uint32_t* d_leaves, int32_t* d_active,
                      void* stream) {
    int16_t* pend = (int16_t*)((char*)ws + rounds_offset(n_cap, S));
    puct_select_batch_kernel<<<n, WAVE, 2 * ((size_t)S + 1), as_stream(stream)>>>((char*)ws, n, S, K, pend, d_leaves,
                                                                                   d_active);
    return gz_check_launch("puct_select_batch_kernel");
}

int backup_batch_impl(void* ws, int32_t n_cap, int32_t n, int32_t S, int32_t K, const double* d_prior,
                      const float* d_value, const PuctNoise& nz, void* stream) {
    int16_t* pend = (int16_t*)((char*)ws + rounds_offset(n_cap, S));
    puct_backup_batch_kernel<<<n, WAVE, 0, as_stream(stream)>>>((char*)ws, n, S, K, pend, d_prior, d_value, nz);
    return gz_check_launch("puct_backup_batch_kernel");
}

// gz_puct_begin on a workspace carved for n_cap games, of which the first n begin
int begin_impl(const gz_board_state* d_boards, const int64_t* d_game_ids, int32_t n_cap, int32_t n,
               const gz_puct_params* p, void* d_workspace, uint32_t* d_leaves, int32_t* d_active, void* stream) {
    if (!p) return gz_fail(GZ_ERR_ARG, "gz_puct_begin: params is NULL");
    int rc = check_S("gz_puct_begin", n, p->num_simulations);
    if (rc) return rc;
    PuctNoise nz;
    rc = read_noise("gz_puct_begin", p, nz);
    if (rc) return rc;
    int K;
    rc = read_leaves("gz_puct_begin", p, K);
    if (rc) return rc;
    rc = check_rows("gz_puct_begin", n_cap, K);
    if (rc) return rc;
    PuctCap cap;
    rc = read_cap("gz_puct_begin", p, cap);
    if (rc) return rc;
    if (n > 0 && (!d_boards || !d_game_ids || !d_workspace || !d_leaves || !d_active))
        return gz_fail(GZ_ERR_ARG, "gz_puct_begin: bad arguments");
    if (n == 0) return GZ_OK;
    note_leaves(d_workspace, K);
    int16_t* pend = K > 0 ? (int16_t*)((char*)d_workspace + rounds_offset(n_cap, p->num_simulations)) : nullptr;
    puct_begin_kernel<<<n, WAVE, 0, as_stream(stream)>>>(d_boards, d_game_ids, n, *p, nz, cap, K, pend,
                                                         (char*)d_workspace, d_leaves, d_active);
    return gz_check_launch("puct_begin_kernel");
}

// The batched search: the root round, ceil(S/K) rounds of n K rows, then one int32 read
// back -- the largest remaining count -- and ceil(left/K) more rounds until it is 0.
// Every unfinished game completes at least one simulation per round, so the count falls.
int search_batch_impl(const gz_board_state* d_boards, const int64_t* d_game_ids, int32_t n_cap, int32_t n,
                      const gz_puct_params* p, int32_t K, const float* d_pv_weights, void* ws, int32_t* d_moves,
                      int32_t* d_visits, double* d_root_q, gz_search_stats* d_stats, void* stream) {
    const int S = p->num_simulations;
    const BatchBufs b = carve_batch(ws, n_cap, S, K);
    const RoundBufs& r = b.r;
    const LeafSym ls = leaf_sym(p, ws, gz_puct_batch_workspace_bytes(n_cap, S, K));
    hipStream_t st = as_stream(stream);
    PuctNoise nz;
    int rc = read_noise("gz_puct_search", p, nz);
    if (rc) return rc;
    rc = begin_impl(d_boards, d_game_ids, n_cap, n, p, ws, r.leaves, r.active, stream);
    if (rc) return rc;
    int todo = 1 + (S + K - 1) / K;
    bool root = true;
    while (todo > 0) {
        for (int round = 0; round < todo; round++) {
            if (!root) {
                rc = select_batch_impl(ws, n_cap, n, S, K, r.leaves, r.active, stream);
                if (rc) return rc;
            }
            root = false;
            rc = sym_leaves(ls, r.leaves, n * K, stream);
            if (rc) return rc;
            rc = gz_pv_forward(d_pv_weights, r.leaves, n * K, nullptr, r.logits, r.value, r.probs, r.prior, r.pvws,
                               p->precision, stream);
            if (rc) return rc;
            rc = sym_priors(ls, r.prior, n * K, stream);
            if (rc) return rc;
            rc = backup_batch_impl(ws, n_cap, n, S, K, r.prior, r.value, nz, stream);
            if (rc) return rc;
        }
        int32_t left = 0;
        hipError_t e = hipMemsetAsync(b.left, 0, sizeof(int32_t), st);
        if (e == hipSuccess) {
            puct_remaining_kernel<<<(n + 255) / 256, 256, 0, st>>>((char*)ws, n, S, nullptr, b.left);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(&left, b.left, sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess)
            return gz_fail(GZ_ERR_HIP, std::string("gz_puct_search: the remaining count: ") + hipGetErrorString(e));
        todo = (left + K - 1) / K;
    }
    return finish_impl(ws, n, S, d_moves, d_visits, d_root_q, d_stats, stream);
}

// The search of the first n games on a workspace sized and carved for n_cap (n <= n_cap):
// every grid, the forward's rows and the remaining count cover those n games only.
int search_impl(const gz_board_state* d_boards, const int64_t* d_game_ids, int32_t n_cap, int32_t n,
                const gz_puct_params* p, const float* d_pv_weights, void* ws, int32_t* d_moves, int32_t* d_visits,
                double* d_root_q, gz_search_stats* d_stats, void* stream) {
    int K = 0;
    if (p->flags & GZ_PUCT_LEAF_BATCH) {
        int rc = read_leaves("gz_puct_search", p, K);
        if (rc) return rc;
        return search_batch_impl(d_boards, d_game_ids, n_cap, n, p, K, d_pv_weights, ws, d_moves, d_visits, d_root_q,
                                 d_stats, stream);
    }
    const int S = p->num_simulations;
    const RoundBufs r = carve_rounds(ws, n_cap, S);
    const LeafSym ls = leaf_sym(p, ws, gz_puct_workspace_bytes(n_cap, S));
    PuctNoise nz;
    int rc = read_noise("gz_puct_search", p, nz);
    if (rc) return rc;
    rc = begin_impl(d_boards, d_game_ids, n_cap, n, p, ws, r.leaves, r.active, stream);
    if (rc) return rc;
    for (int round = 0; round <= S; round++) {
        if (round > 0) {
            rc = gz_puct_select(ws, n, S, r.leaves, r.active, stream);
            if (rc) return rc;
        }
        rc = sym_leaves(ls, r.leaves, n, stream);
        if (rc) return rc;
        rc = gz_pv_forward(d_pv_weights, r.leaves, n, nullptr, r.logits, r.value, r.probs, r.prior, r.pvws,
                           p->precision, stream);
        if (rc) return rc;
        rc = sym_priors(ls, r.prior, n, stream);
        if (rc) return rc;
        rc = backup_impl(ws, n, S, r.prior, r.value, nz, stream);
        if (rc) return rc;
    }
    return finish_impl(ws, n, S, d_moves, d_visits, d_root_q, d_stats, stream);
}

int check_search_args(const char* who, const gz_puct_params* p, int32_t n) {
    if (!p) return gz_fail(GZ_ERR_ARG, std::string(who) + ": params is NULL");
    int rc = check_S(who, n, p->num_simulations);
    if (rc) return rc;
    if (p->precision != GZ_PV_FP32 && p->precision != GZ_PV_F16X3 && p->precision != GZ_PV_F16)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": unknown precision");
    PuctNoise nz;
    rc = read_noise(who, p, nz);
    if (rc) return rc;
    int K;
    rc = read_leaves(who, p, K);
    if (rc) return rc;
    PuctCap cap;
    rc = read_cap(who, p, cap);
    if (rc) return rc;
    return check_rows(who, n, K);
}

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

size_t pend_bytes(int32_t n_slots) { return al256((size_t)n_slots * GZ_MAX_GAME_PLIES * GZ_CELLS * 2); }

SelfplayWs carve_selfplay(void* ws, int32_t n) {
    char* p = (char*)ws;
    SelfplayWs w;
    w.boards = (gz_board_state*)p;
    p += al256((size_t)n * sizeof(gz_board_state));
    w.gids = (int64_t*)p;
    p += al256((size_t)n * 8);
    w.moves = (int32_t*)p;
    p += al256((size_t)n * 4);
    w.stats = (gz_search_stats*)p;
    p += al256((size_t)n * sizeof(gz_search_stats));
    w.visits = (int32_t*)p;
    p += al256((size_t)n * 900);
    w.root_q = (double*)p;
    p += al256((size_t)n * 8);
    w.pend = (uint16_t*)p;
    p += pend_bytes(n);
    w.puct = p;
    return w;
}

// gz_selfplay_puct_run(_active): n_slots sized and carved the workspace, the first n plays
int run_impl(const char* who, void* d_slots, int32_t n_slots, int32_t n, const gz_puct_params* p,
             const float* d_pv_weights, void* d_workspace, int32_t n_plies, gz_record* d_records, int32_t record_cap,
             uint16_t* d_visits, gz_selfplay_counters* d_counters, void* stream) {
    int rc = check_search_args(who, p, n_slots);
    if (rc) return rc;
    if (!d_slots || n_slots <= 0 || n_plies < 0 || !d_counters || !d_records || record_cap < 0 || !d_workspace ||
        !d_pv_weights || !d_visits)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": bad arguments");
    if (n < 1 || n > n_slots) return gz_fail(GZ_ERR_ARG, std::string(who) + ": n_active out of range [1, n_slots]");
    const SelfplayWs w = carve_selfplay(d_workspace, n_slots);
    hipStream_t st = as_stream(stream);
    for (int it = 0; it < n_plies; it++) {
        rc = gz_selfplay_boards(d_slots, n, p->num_simulations, w.boards, w.gids, stream);
        if (rc) return rc;
        rc = search_impl(w.boards, w.gids, n_slots, n, p, d_pv_weights, w.puct, w.moves, w.visits, w.root_q, w.stats,
                         stream);
        if (rc) return rc;
        puct_stash_kernel<<<n, WAVE, 0, st>>>(w.boards, w.moves, w.visits, n, w.pend);
        rc = gz_check_launch("puct_stash_kernel");
        if (rc) return rc;
        rc = gz_internal_selfplay_commit(d_slots, n, w.moves, w.stats, d_records, record_cap, d_counters, w.pend,
                                         d_visits, stream);
        if (rc) return rc;
    }
    return GZ_OK;
}

// gz_selfplay_puct_rounds(_active), as run_impl
int rounds_impl(const char* who, void* d_slots, int32_t n_slots, int32_t n, const gz_puct_params* p,
                const float* d_pv_weights, void* d_workspace, int32_t n_rounds, gz_record* d_records,
                int32_t record_cap, uint16_t* d_visits, gz_selfplay_counters* d_counters, void* stream) {
    int rc = check_search_args(who, p, n_slots);
    if (rc) return rc;
    if (!d_slots || n_slots <= 0 || n_rounds < 0 || !d_counters || !d_records || record_cap < 0 || !d_workspace ||
        !d_pv_weights || !d_visits)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": bad arguments");
    int K;
    rc = read_leaves(who, p, K);
    if (rc) return rc;
    if (K > 1)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": tree reuse with leaves_per_round > 1 is not supported");
    if (n < 1 || n > n_slots) return gz_fail(GZ_ERR_ARG, std::string(who) + ": n_active out of range [1, n_slots]");
    const int S = p->num_simulations;
    const SelfplayWs w = carve_selfplay(d_workspace, n_slots);
    const RoundBufs r = carve_rounds(w.puct, n_slots, S);
    const LeafSym ls = leaf_sym(p, w.puct, gz_puct_workspace_bytes(n_slots, S));
    hipStream_t st = as_stream(stream);
    PuctNoise nz;
    rc = read_noise(who, p, nz);
    if (rc) return rc;
    PuctCap cap;
    rc = read_cap(who, p, cap);
    if (rc) return rc;
    for (int it = 0; it < n_rounds; it++) {
        puct_advance_kernel<<<n, RR_THREADS, remap_bytes(S), st>>>((const char*)d_slots, n, *p, nz, cap,
                                                                   (char*)w.puct, w.moves, w.stats, w.pend);
        rc = gz_check_launch("puct_advance_kernel");
        if (rc) return rc;
        rc = gz_internal_selfplay_commit(d_slots, n, w.moves, w.stats, d_records, record_cap, d_counters, w.pend,
                                         d_visits, stream);
        if (rc) return rc;
        puct_round_kernel<<<n, WAVE, 0, st>>>((const char*)d_slots, n, *p, cap, (char*)w.puct, r.leaves, r.active);
        rc = gz_check_launch("puct_round_kernel");
        if (rc) return rc;
        rc = sym_leaves(ls, r.leaves, n, stream);
        if (rc) return rc;
        rc = gz_pv_forward(d_pv_weights, r.leaves, n, nullptr, r.logits, r.value, r.probs, r.prior, r.pvws,
                           p->precision, stream);
        if (rc) return rc;
        rc = sym_priors(ls, r.prior, n, stream);
        if (rc) return rc;
        rc = backup_impl(w.puct, n, S, r.prior, r.value, nz, stream);
        if (rc) return rc;
    }
    return GZ_OK;
}

// the match workspace after the self-play workspace of n slots: side i32 [n], row_of i32
// [n], the two counts (256 bytes), then per side the round buffers of n rows
struct MatchWs {
    int32_t *side, *row_of, *count;
    RoundBufs pk[2];
};

size_t rows_bytes(int32_t n) {
    const size_t m = (size_t)n;
    return al256(m * 64) + al256(m * 4) + 2 * al256(m * 900) + al256(m * 4) + al256(m * 1800) + gz_pv_workspace_bytes(n);
}

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

bool known_precision(int32_t x) { return x == GZ_PV_FP32 || x == GZ_PV_F16X3 || x == GZ_PV_F16; }

// gz_puct_match_run: run_impl with the routed evaluation in place of the one forward
int match_impl(void* d_slots, int32_t n_slots, int32_t n, const gz_puct_match_params* mp, void* d_workspace,
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
    PuctNoise nz;
    rc = read_noise(who, p, nz);
    if (rc) return rc;
    if (!known_precision(mp->precision[0]) || !known_precision(mp->precision[1]))
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": unknown precision");
    if (mp->a_black_parity != 0 && mp->a_black_parity != 1)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": a_black_parity must be 0 or 1");
    if (!d_slots || n_slots <= 0 || n_plies < 0 || !d_counters || !d_records || record_cap < 0 || !d_workspace ||
        !mp->d_weights[0] || !mp->d_weights[1] || !d_visits)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": bad arguments");
    if (n < 1 || n > n_slots) return gz_fail(GZ_ERR_ARG, std::string(who) + ": n_active out of range [1, n_slots]");
    const int S = p->num_simulations;
    const SelfplayWs w = carve_selfplay(d_workspace, n_slots);
    const RoundBufs r = carve_rounds(w.puct, n_slots, S);
    const MatchWs m = carve_match(d_workspace, n_slots, S);
    // (both sides under the same t: the slot rows turn before the gather and back after the scatter)
    const LeafSym ls = leaf_sym(p, d_workspace, gz_puct_match_workspace_bytes(n_slots, S));
    hipStream_t st = as_stream(stream);
    for (int it = 0; it < n_plies; it++) {
        rc = gz_selfplay_boards(d_slots, n, S, w.boards, w.gids, stream);
        if (rc) return rc;
        puct_match_plan_kernel<<<1, 1024, 0, st>>>((const char*)d_slots, n, mp->a_black_parity, w.boards, m.side,
                                                   m.row_of, m.count);
        rc = gz_check_launch("puct_match_plan_kernel");
        if (rc) return rc;
        rc = begin_impl(w.boards, w.gids, n_slots, n, p, w.puct, r.leaves, r.active, stream);
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
            rc = backup_impl(w.puct, n, S, r.prior, r.value, nz, stream);
            if (rc) return rc;
        }
        rc = finish_impl(w.puct, n, S, w.moves, w.visits, w.root_q, w.stats, stream);
        if (rc) return rc;
        puct_stash_kernel<<<n, WAVE, 0, st>>>(w.boards, w.moves, w.visits, n, w.pend);
        rc = gz_check_launch("puct_stash_kernel");
        if (rc) return rc;
        rc = gz_internal_selfplay_commit(d_slots, n, w.moves, w.stats, d_records, record_cap, d_counters, w.pend,
                                         d_visits, stream);
        if (rc) return rc;
    }
    return GZ_OK;
}

}  // namespace

extern "C" {

size_t gz_puct_tree_bytes(int32_t S) { return S < 0 ? 0 : export_bytes_for(S); }

size_t gz_puct_workspace_bytes(int32_t n, int32_t S) {
    if (n < 1) n = 1;
    if (S < 0) S = 0;
    const size_t m = (size_t)n;
    return rounds_offset(n, S) + al256(m * 64) + al256(m * 4) + 2 * al256(m * 900) + al256(m * 4) + al256(m * 1800) +
           gz_pv_workspace_bytes(n);
}

int gz_puct_begin(const gz_board_state* d_boards, const int64_t* d_game_ids, int32_t n, const gz_puct_params* p,
                  void* d_workspace, uint32_t* d_leaves, int32_t* d_active, void* stream) {
    return begin_impl(d_boards, d_game_ids, n, n, p, d_workspace, d_leaves, d_active, stream);
}

int gz_puct_select(void* d_workspace, int32_t n, int32_t S, uint32_t* d_leaves, int32_t* d_active, void* stream) {
    int rc = check_S("gz_puct_select", n, S);
    if (rc) return rc;
    if (n > 0 && (!d_workspace || !d_leaves || !d_active)) return gz_fail(GZ_ERR_ARG, "gz_puct_select: bad arguments");
    if (n == 0) return GZ_OK;
    const int K = leaves_of(d_workspace);
    if (K > 0) return select_batch_impl(d_workspace, n, n, S, K, d_leaves, d_active, stream);
    puct_select_kernel<<<n, WAVE, 0, as_stream(stream)>>>((char*)d_workspace, n, S, d_leaves, d_active);
    return gz_check_launch("puct_select_kernel");
}

int gz_puct_backup(void* d_workspace, int32_t n, int32_t S, const double* d_prior, const float* d_value,
                   void* stream) {
    int rc = check_S("gz_puct_backup", n, S);
    if (rc) return rc;
    if (n > 0 && (!d_workspace || !d_prior || !d_value)) return gz_fail(GZ_ERR_ARG, "gz_puct_backup: bad arguments");
    if (n == 0) return GZ_OK;
    PuctNoise nz = {};
    nz.on = -1;  // as gz_puct_begin stored it in the workspace
    const int K = leaves_of(d_workspace);
    if (K > 0) return backup_batch_impl(d_workspace, n, n, S, K, d_prior, d_value, nz, stream);
    return backup_impl(d_workspace, n, S, d_prior, d_value, nz, stream);
}

int gz_puct_remaining(void* d_workspace, int32_t n, int32_t S, int32_t* d_remaining, void* stream) {
    int rc = check_S("gz_puct_remaining", n, S);
    if (rc) return rc;
    if (n > 0 && (!d_workspace || !d_remaining)) return gz_fail(GZ_ERR_ARG, "gz_puct_remaining: bad arguments");
    if (n == 0) return GZ_OK;
    puct_remaining_kernel<<<(n + 255) / 256, 256, 0, as_stream(stream)>>>((char*)d_workspace, n, S, d_remaining,
                                                                         nullptr);
    return gz_check_launch("puct_remaining_kernel");
}

size_t gz_puct_sym_bytes(int32_t rows) { return al256((size_t)(rows < 1 ? 1 : rows)); }

size_t gz_puct_batch_workspace_bytes(int32_t n, int32_t S, int32_t K) {
    if (n < 1) n = 1;
    if (S < 0) S = 0;
    if (K < 1) K = 1;
    if (K > GZ_PUCT_MAX_LEAVES) K = GZ_PUCT_MAX_LEAVES;
    const size_t m = (size_t)n * K;
    return rounds_offset(n, S) + batch_pend_bytes(n, K) + 256 + al256(m * 64) + al256(m * 4) + 2 * al256(m * 900) +
           al256(m * 4) + al256(m * 1800) + gz_pv_workspace_bytes((int32_t)m);
}

int gz_puct_finish(void* d_workspace, int32_t n, int32_t S, int32_t* d_moves, int32_t* d_visits, double* d_root_q,
                   void* stream) {
    int rc = check_S("gz_puct_finish", n, S);
    if (rc) return rc;
    if (n > 0 && (!d_workspace || !d_moves)) return gz_fail(GZ_ERR_ARG, "gz_puct_finish: bad arguments");
    if (n == 0) return GZ_OK;
    return finish_impl(d_workspace, n, S, d_moves, d_visits, d_root_q, nullptr, stream);
}

int gz_puct_search(const gz_board_state* d_boards, const int64_t* d_game_ids, int32_t n, const gz_puct_params* p,
                   const float* d_pv_weights, void* d_workspace, int32_t* d_moves, int32_t* d_visits,
                   double* d_root_q, void* stream) {
    int rc = check_search_args("gz_puct_search", p, n);
    if (rc) return rc;
    if (n > 0 && (!d_boards || !d_game_ids || !d_pv_weights || !d_workspace || !d_moves))
        return gz_fail(GZ_ERR_ARG, "gz_puct_search: bad arguments");
    if (n == 0) return GZ_OK;
    return search_impl(d_boards, d_game_ids, n, n, p, d_pv_weights, d_workspace, d_moves, d_visits, d_root_q, nullptr,
                       stream);
}

int gz_puct_trees(const void* d_workspace, int32_t n, int32_t S, void* d_out, void* stream) {
    int rc = check_S("gz_puct_trees", n, S);
    if (rc) return rc;
    if (n > 0 && (!d_workspace || !d_out)) return gz_fail(GZ_ERR_ARG, "gz_puct_trees: bad arguments");
    if (n == 0) return GZ_OK;
    puct_export_kernel<<<n, 256, 0, as_stream(stream)>>>((const char*)d_workspace, n, S, (char*)d_out);
    return gz_check_launch("puct_export_kernel");
}

size_t gz_selfplay_puct_workspace_bytes(int32_t n_slots, int32_t S) {
    if (n_slots < 1) n_slots = 1;
    const size_t m = (size_t)n_slots;
    return al256(m * sizeof(gz_board_state)) + al256(m * 8) + al256(m * 4) + al256(m * sizeof(gz_search_stats)) +
           al256(m * 900) + al256(m * 8) + pend_bytes(n_slots) + gz_puct_workspace_bytes(n_slots, S);
}

size_t gz_selfplay_puct_batch_workspace_bytes(int32_t n_slots, int32_t S, int32_t K) {
    if (n_slots < 1) n_slots = 1;
    const size_t m = (size_t)n_slots;
    return al256(m * sizeof(gz_board_state)) + al256(m * 8) + al256(m * 4) + al256(m * sizeof(gz_search_stats)) +
           al256(m * 900) + al256(m * 8) + pend_bytes(n_slots) + gz_puct_batch_workspace_bytes(n_slots, S, K);
}

int gz_selfplay_puct_run_active(void* d_slots, int32_t n_slots, int32_t n_active, const gz_puct_params* p,
                                const float* d_pv_weights, void* d_workspace, int32_t n_plies, gz_record* d_records,
                                int32_t record_cap, uint16_t* d_visits, gz_selfplay_counters* d_counters,
                                void* stream) {
    return run_impl("gz_selfplay_puct_run_active", d_slots, n_slots, n_active, p, d_pv_weights, d_workspace, n_plies,
                    d_records, record_cap, d_visits, d_counters, stream);
}

int gz_selfplay_puct_run(void* d_slots, int32_t n_slots, const gz_puct_params* p, const float* d_pv_weights,
                         void* d_workspace, int32_t n_plies, gz_record* d_records, int32_t record_cap,
                         uint16_t* d_visits, gz_selfplay_counters* d_counters, void* stream) {
    return run_impl("gz_selfplay_puct_run", d_slots, n_slots, n_slots, p, d_pv_weights, d_workspace, n_plies, d_records,
                    record_cap, d_visits, d_counters, stream);
}

int gz_puct_reroot(void* d_workspace, int32_t n, int32_t S, const int32_t* d_moves, uint32_t* d_leaves,
                   int32_t* d_active, int32_t* d_remaining, void* stream) {
    int rc = check_S("gz_puct_reroot", n, S);
    if (rc) return rc;
    if (n > 0 && (!d_workspace || !d_moves || !d_leaves || !d_active))
        return gz_fail(GZ_ERR_ARG, "gz_puct_reroot: bad arguments");
    if (n == 0) return GZ_OK;
    if (leaves_of(d_workspace) > 1)
        return gz_fail(GZ_ERR_ARG, "gz_puct_reroot: tree reuse with leaves_per_round > 1 is not supported");
    puct_reroot_kernel<<<n, RR_THREADS, remap_bytes(S), as_stream(stream)>>>((char*)d_workspace, n, S, d_moves, d_leaves,
                                                                      d_active, d_remaining);
    return gz_check_launch("puct_reroot_kernel");
}

int gz_selfplay_puct_reset(void* d_workspace, int32_t n_slots, int32_t S, void* stream) {
    int rc = check_S("gz_selfplay_puct_reset", n_slots, S);
    if (rc) return rc;
    if (!d_workspace || n_slots <= 0) return gz_fail(GZ_ERR_ARG, "gz_selfplay_puct_reset: bad arguments");
    const SelfplayWs w = carve_selfplay(d_workspace, n_slots);
    puct_reset_kernel<<<(n_slots + 255) / 256, 256, 0, as_stream(stream)>>>((char*)w.puct, n_slots, S);
    return gz_check_launch("puct_reset_kernel");
}

int gz_selfplay_puct_rounds_active(void* d_slots, int32_t n_slots, int32_t n_active, const gz_puct_params* p,
                                   const float* d_pv_weights, void* d_workspace, int32_t n_rounds,
                                   gz_record* d_records, int32_t record_cap, uint16_t* d_visits,
                                   gz_selfplay_counters* d_counters, void* stream) {
    return rounds_impl("gz_selfplay_puct_rounds_active", d_slots, n_slots, n_active, p, d_pv_weights, d_workspace,
                       n_rounds, d_records, record_cap, d_visits, d_counters, stream);
}

int gz_selfplay_puct_rounds(void* d_slots, int32_t n_slots, const gz_puct_params* p, const float* d_pv_weights,
                            void* d_workspace, int32_t n_rounds, gz_record* d_records, int32_t record_cap,
                            uint16_t* d_visits, gz_selfplay_counters* d_counters, void* stream) {
    return rounds_impl("gz_selfplay_puct_rounds", d_slots, n_slots, n_slots, p, d_pv_weights, d_workspace, n_rounds,
                       d_records, record_cap, d_visits, d_counters, stream);
}

int gz_selfplay_puct_layout(int32_t n_slots, int32_t S, int32_t K, size_t out[4]) {
    int rc = check_S("gz_selfplay_puct_layout", n_slots, S);
    if (rc) return rc;
    if (n_slots < 1 || K < 0 || K > GZ_PUCT_MAX_LEAVES || !out)
        return gz_fail(GZ_ERR_ARG, "gz_selfplay_puct_layout: bad arguments");
    const uintptr_t base = 4096;  // (any address: only the differences are used)
    const SelfplayWs w = carve_selfplay((void*)base, n_slots);
    out[0] = (size_t)((uintptr_t)w.pend - base);
    out[1] = (size_t)((uintptr_t)w.puct - base);
    out[2] = out[1] + 256;
    out[3] = game_stride_for(S);
    return GZ_OK;
}

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
    if (n_active < 1 || n_active > n_slots)
        return gz_fail(GZ_ERR_ARG, "gz_selfplay_puct_compact: n_active out of range [1, n_slots]");
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

size_t gz_puct_match_workspace_bytes(int32_t n_slots, int32_t S) {
    if (n_slots < 1) n_slots = 1;
    return gz_selfplay_puct_workspace_bytes(n_slots, S) + 2 * al256((size_t)n_slots * 4) + 256 + 2 * rows_bytes(n_slots);
}

int gz_puct_match_run(void* d_slots, int32_t n_slots, int32_t n_active, const gz_puct_match_params* mp,
                      void* d_workspace, int32_t n_plies, gz_record* d_records, int32_t record_cap,
                      uint16_t* d_visits, gz_selfplay_counters* d_counters, void* stream) {
    return match_impl(d_slots, n_slots, n_active, mp, d_workspace, n_plies, d_records, record_cap, d_visits,
                      d_counters, stream);
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

int gz_puct_root_noise(const gz_board_state* d_boards, const int64_t* d_game_ids, int32_t n, uint64_t seed,
                       double alpha, double* d_eta, void* stream) {
    int rc = check_alpha("gz_puct_root_noise", alpha);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!d_boards || !d_game_ids || !d_eta)))
        return gz_fail(GZ_ERR_ARG, "gz_puct_root_noise: bad arguments");
    if (n == 0) return GZ_OK;
    puct_root_noise_kernel<<<n, WAVE, 0, as_stream(stream)>>>(d_boards, d_game_ids, n, seed, alpha, d_eta);
    return gz_check_launch("puct_root_noise_kernel");
}

int gz_puct_cap_full(const gz_record* d_records, int32_t n, uint64_t seed, double full_prob, uint8_t* d_full,
                     void* stream) {
    int rc = check_full_prob("gz_puct_cap_full", full_prob);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!d_records || !d_full))) return gz_fail(GZ_ERR_ARG, "gz_puct_cap_full: bad arguments");
    if (n == 0) return GZ_OK;
    puct_cap_full_kernel<<<(n + 255) / 256, 256, 0, as_stream(stream)>>>(d_records, n, seed, full_prob, d_full);
    return gz_check_launch("puct_cap_full_kernel");
}

int gz_puct_cap_full_host(uint64_t seed, int64_t game_id, int32_t ply, double full_prob) {
    return cap_is_full(seed, game_id, ply, full_prob) ? 1 : 0;
}

int gz_puct_root_noise_host(uint64_t seed, int64_t game_id, int32_t ply, const uint8_t* empty225, double alpha,
                            double* eta225) {
    int rc = check_alpha("gz_puct_root_noise_host", alpha);
    if (rc) return rc;
    if (!empty225 || !eta225) return gz_fail(GZ_ERR_ARG, "gz_puct_root_noise_host: bad arguments");
    noise_eta_row(stream_key(seed, game_id, ply, GZ_NOISE_SIM), empty225, alpha, eta225);
    return GZ_OK;
}

}  // extern "C"
