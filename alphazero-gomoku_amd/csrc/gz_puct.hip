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
// Forced playouts and policy-target pruning (opt-in, GZ_PUCT_FORCED_PLAYOUTS; gz_forced.h,
// tests/puct_forced_ref.py restates it).  At a root whose budget is S a child with n >= 1
// visits scores +infinity while n < sqrt((k * prior[0][c]) * (visits[0] - 1))
// (descend_once<false, true>, reached for i == 0 only), and the visit row that leaves the
// search -- puct_finish_kernel's d_visits, the row puct_advance_kernel stashes -- gives back
// the forced playouts a child would not hold by PUCT (prune_row, between pick_move and the
// row stores; the move and the exported tree keep the raw counts).  The flag-clear kernels
// are untouched: the forced paths are kernels of their own (puct_select_forced_kernel,
// puct_round_forced_kernel, puct_finish_forced_kernel, puct_advance_forced_kernel), chosen
// on the host from the params or, in the step API, from what gz_puct_begin noted for the
// workspace.  k = 0 is the flag clear.  Not with leaf batching, not in a match.
//
// Gumbel root with sequential halving (opt-in, GZ_PUCT_GUMBEL; gz_gumbel.h,
// tests/puct_gumbel_ref.py restates it).  When node 0's evaluation is stored
// (puct_backup_gumbel_kernel) the root's considered cells are drawn without replacement by
// the Gumbel-top-k trick -- m rounds of wave_argmax over g(c) + logit(c) -- and their scores
// kept in gs f64 [225], -infinity elsewhere.  puct_select_gumbel_kernel picks the root's cell
// by the halving schedule (the considered child with seq(m, S)[visits[0] - 1] visits and the
// best gs + sigma(q)) and descends by PUCT below it (descend_once<false, false, true>);
// puct_finish_gumbel_kernel picks the move among the most-visited considered cells and hands
// out softmax(logits + sigma(completed q)) scaled to 32767 as the row.  A search is still S+1
// rounds.  The flag-clear and forced kernels are untouched: the host chooses these three from
// the params or, in the step API, from what gz_puct_begin noted for the workspace.  gs and the
// schedule tables lie behind the flag-clear workspace.  Not with root noise, leaf batching, the
// playout cap, forced playouts or tree reuse, not in a match.
//
// The layouts (workspace, export, self-play) are in gz_puct.h, which the PUCT units share;
// slot compaction is gz_puct_compact.hip, the match gz_puct_match.hip.
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
//
// Leaf symmetry (opt-in, GZ_PUCT_LEAF_SYM; gz_sym.h, gz_pvsym.hip, tests/puct_sym_ref.py):
// every leaf is evaluated on its board under t = sym_of(seed, leaf row), one of the 8
// symmetries, and the prior row is mapped back; the value is a scalar.  Two launches per
// round around the forward, in all five paths:
//   select / begin / round -> sym_leaves (leaf rows in place, t per row) -> gz_pv_forward
//   -> sym_priors (the f64 prior rows in place) -> backup (the root noise as ever, on the
//   mapped-back row);
// the match (gz_puct_match.hip) likewise.  The select, backup, re-root and compaction kernels do
// not know about it.  t lives behind the flag-clear workspace: gz_puct_sym_bytes(rows) more
// bytes, touched only with the flag set.
// The step API accepts the flag and ignores it (its caller evaluates: gz_pv_forward_sym).
#include <hip/hip_runtime.h>

#include <climits>
#include <mutex>
#include <string>
#include <unordered_map>

#include "gz_dirichlet.h"
#include "gz_puct.h"

using namespace gz;

namespace {

// the root noise of a launch: nz, or (on < 0) what gz_puct_begin stored in the PuctCfg
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

// the playout cap of a launch, as noise_of
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

__device__ inline int budget_of(const PuctCap& cap, bool full, int S) { return full ? S : cap.fast; }

// the budget of an inherited root, right after reroot() (every lane of one wave calls;
// the header already holds the new ply); returns whether the ply is full
__device__ inline bool set_budget(PuctHdr* h, const PuctCap& cap, uint64_t seed, int S) {
    const bool full = root_is_full(cap, seed, h->game_id, h->n_moves);
    if (lane_id() == 0) {
        h->budget = budget_of(cap, full, S);
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
    begin_root(t, black, white, game_ids[g], bs.n_moves, bs.player, over, 0, budget_of(cap, full, S), full);
    write_leaf(leaves, active, g * rows, black, white, !over);
    for (int k = 1; k < rows; k++) write_leaf(leaves, active, g * rows + k, black, white, false);
    if (pend)
        for (int k = lane; k < rows; k += WAVE) pend[(size_t)g * rows + k] = -1;
}

// ---------------------------------------------------------------- select
// What one descent did.  NONE: the tree is as it was (no empty cell, no node left, a
// collision).  TERMINAL: a terminal node, found on the path or created, was backed up.
// LEAF: node j was created under `parent` and waits for its evaluation.
enum { DESCENT_NONE, DESCENT_TERMINAL, DESCENT_LEAF };

struct Descent {
    int what;
    int j, parent;
};

// One descent by PUCT from the root -- position black / white, `mover` to move at ply cnt --
// to a new child, which it creates; black / white leave as the position where it ended.
// VL: virtual loss is in play (the header comment has both forms of the score).  vl [S+1]
// counts the leaves of this launch that wait below a node, and a live child created in this
// launch (index >= first) has no prior row yet: a collision.  Without VL neither is read.
// FORCED (GZ_PUCT_FORCED_PLAYOUTS, gz_forced.h; never with VL): at the root a visited child
// that is short of forced_min(forced_k, prior, visits[0] - 1) visits scores +infinity; the
// first-maximum rule picks among several.  forced_k = 0 (a fast ply's root) forces nothing.
// Without FORCED forced_k is not read.
// GUMBEL (GZ_PUCT_GUMBEL; never with VL or FORCED): the root's cell is root_cell, chosen by the
// caller (gumbel_root_cell); below the root the descent is the one above.
template <bool VL, bool FORCED = false, bool GUMBEL = false>
__device__ inline Descent descend_once(const PuctTree& t, double c_puct, int S, const int16_t* vl, int first,
                                       BB& black, BB& white, int mover, int cnt, double forced_k = 0.0,
                                       int root_cell = -1) {
    static_assert(!(VL && FORCED), "forced playouts are not defined with virtual loss");
    static_assert(!(GUMBEL && (VL || FORCED)), "the Gumbel root stands alone");
    const int lane = lane_id();
    PuctHdr* h = t.h;
    int i = 0;
    while (true) {
        const int tm = t.term[i];
        if (tm) {
            if (lane == 0) backup(t, i, tm == 3 ? 0.0 : -1.0);
            return {DESCENT_TERMINAL, i, -1};
        }
        const BB E = empties(black, white);
        int ni = t.visits[i];
        if constexpr (VL) ni += vl[i];
        const double sq = __builtin_sqrt((double)ni);
        const double* pr = t.prior + (size_t)i * GZ_CELLS;
        const int16_t* ch = t.child + (size_t)i * GZ_CELLS;
        double bv = -__builtin_inf();
        int bi = INT_MAX;
        bool chosen = false;
        if constexpr (GUMBEL) {
            if (i == 0) {
                bi = root_cell;
                chosen = true;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = lane + WAVE * k;
            if (!chosen && c < GZ_CELLS && bb_test(E, cell_to_bit(c))) {
                const int cj = ch[c];
                int nn = 0;
                double q = 0.0;
                if (cj >= 0) {
                    if constexpr (VL) {
                        const int lost = vl[cj];
                        nn = t.visits[cj] + lost;
                        q = nn ? (t.W[cj] - (double)lost) / (double)nn : 0.0;
                    } else {
                        nn = t.visits[cj];
                        q = nn ? t.W[cj] / (double)nn : 0.0;
                    }
                }
                const double u = ((c_puct * pr[c]) * sq) / (1.0 + (double)nn);
                double sc = q + u;
                if constexpr (FORCED)
                    if (i == 0 && nn >= 1 && (double)nn < forced_min(forced_k, pr[c], ni - 1)) sc = __builtin_inf();
                if (sc > bv) {
                    bv = sc;
                    bi = c;
                }
            }
        }
        if (!chosen) wave_argmax(bv, bi);
        if (bi == INT_MAX) bi = bit_to_cell(lowest_bit(E));  // only if the evaluator gave non-finite priors
        if (bi < 0 || bi >= GZ_CELLS) return {DESCENT_NONE, -1, -1};  // (a live node always has an empty cell)
        const int bit = cell_to_bit(bi);
        const int cj = ch[bi];
        if (cj >= 0) {
            if constexpr (VL)
                if (cj >= first && t.term[cj] == 0) return {DESCENT_NONE, -1, -1};  // a collision
            if (mover == 1) bb_set(black, bit);
            else bb_set(white, bit);
            mover = 3 - mover;
            cnt++;
            i = cj;
            continue;
        }
        const int j = h->n_nodes;
        // more select steps than the workspace was sized for: no node left (never within the
        // budget: every descent creates at most one node)
        if (j > S) return {DESCENT_NONE, -1, -1};
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
        }
        return {term ? DESCENT_TERMINAL : DESCENT_LEAF, j, i};
    }
}

// One simulation's descent of game g's tree: the new leaf's board into row g, or an
// empty row (a terminal node backed up, a game that is over, waits for a backup or
// whose root already has its budget's B+1 visits -- with tree reuse, where a game can
// reach its budget before the others, and on the fast plies of a playout cap).
// FORCED: playouts are forced with forced_k at a root whose budget is the full one.
template <bool FORCED = false>
__device__ inline void descend(const PuctTree& t, double c_puct, int S, int g, uint32_t* leaves, int32_t* active,
                               double forced_k = 0.0) {
    PuctHdr* h = t.h;
    BB black, white;
    load_bb(black, h->black);
    load_bb(white, h->white);
    bool live = false;
    // (pending: the caller skipped a backup; keep the tree as it is)
    if (!(h->over || h->pending >= 0 || t.visits[0] > h->budget)) {
        const Descent d = descend_once<false, FORCED>(t, c_puct, S, nullptr, 0, black, white, h->player, h->n_moves,
                                                      h->budget == S ? forced_k : 0.0);
        live = d.what == DESCENT_LEAF;
        if (live && lane_id() == 0) h->pending = d.j;
    }
    write_leaf(leaves, active, g, black, white, live);
}

__global__ __launch_bounds__(WAVE) void puct_select_kernel(char* ws, int n, int S, uint32_t* leaves, int32_t* active) {
    const int g = blockIdx.x;
    if (g >= n) return;
    const PuctCfg cfg = *(const PuctCfg*)ws;
    descend(tree_of(ws, g, S), cfg.c_puct, S, g, leaves, active);
}

// gz_puct_begin with GZ_PUCT_FORCED_PLAYOUTS (k > 0): k beside the configuration the begin
// kernel has just written (stream order), for the forced select and finish kernels -- the
// only ones that read it
__global__ void puct_forced_cfg_kernel(char* ws, double forced_k) {
    ((PuctCfg*)ws)->forced_k = forced_k;
}

// puct_select_kernel of a workspace whose search forces playouts
__global__ __launch_bounds__(WAVE) void puct_select_forced_kernel(char* ws, int n, int S, uint32_t* leaves,
                                                                  int32_t* active) {
    const int g = blockIdx.x;
    if (g >= n) return;
    const PuctCfg cfg = *(const PuctCfg*)ws;
    descend<true>(tree_of(ws, g, S), cfg.c_puct, S, g, leaves, active, cfg.forced_k);
}

// ---------------------------------------------------------------- backup
// Node j receives row `row` of the round buffers: the prior row by the whole wave, the
// value by lane 0, which backs it up.
__device__ inline void store_eval(const PuctTree& t, int j, const double* prior, const float* value, size_t row) {
    const int lane = lane_id();
    for (int c = lane; c < GZ_CELLS; c += WAVE) t.prior[(size_t)j * GZ_CELLS + c] = prior[row * GZ_CELLS + c];
    if (lane == 0) {
        const float v = value[row];
        t.value[j] = v;
        backup(t, j, (double)v);
        t.h->n_evals += 1;
        t.h->new_evals += 1;
    }
}

// The pending node j (>= 0) receives its evaluation.  The root noise is mixed here, into
// the row of a root as it is stored (node 0 pending: gz_puct_begin's, puct_round_kernel's
// and gz_puct_reroot's one-node roots), and not in a kernel of its own: roots appear in any
// round of gz_selfplay_puct_rounds, so a separate kernel would be one more launch in every
// round, while here a round without a new root pays one uniform branch.  (nz by value: a
// reference to the kernel's argument keeps a copy of it in scratch.)
__device__ inline void store_pending_eval(const PuctTree& t, int j, const char* ws, PuctNoise nz, const double* prior,
                                          const float* value, size_t row) {
    store_eval(t, j, prior, value, row);
    if (j == 0 && t.h->full) {  // (a fast ply's root keeps the evaluator's row)
        const PuctNoise z = noise_of(nz, ws);
        if (z.on) mix_root_row(t, z);  // (each lane mixes the cells it has just stored)
    }
    if (lane_id() == 0) t.h->pending = -1;
}

__global__ __launch_bounds__(WAVE) void puct_backup_kernel(char* ws, int n, int S, const double* prior,
                                                           const float* value, PuctNoise nz) {
    const int g = blockIdx.x;
    if (g >= n) return;
    PuctTree t = tree_of(ws, g, S);
    const int j = t.h->pending;
    if (j >= 0) store_pending_eval(t, j, ws, nz, prior, value, g);
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
        const Descent d = descend_once<true>(t, c_puct, S, vl, first, black, white, player0, cnt0);
        if (d.what == DESCENT_NONE) go = false;
        if (d.what == DESCENT_LEAF) {
            if (lane == 0) {
                pd[k] = (int16_t)d.j;
                vl[d.j] += 1;
                for (int x = d.parent; x >= 0; x = t.parent[x]) vl[x] += 1;
            }
            write_leaf(leaves, active, g * K + k, black, white, true);
            k++;
        }
        batch_sync();
    }
    for (; k < K; k++) {
        write_leaf(leaves, active, g * K + k, rblack, rwhite, false);
        if (lane == 0) pd[k] = -1;
    }
}

// The backup step of a batched round: the root of gz_puct_begin (header.pending, row g K),
// else the game's active rows in ascending order -- the prior rows by the whole wave, values
// and backups by lane 0 one row after the other, so every W sums in the reference's order.
__global__ __launch_bounds__(WAVE) void puct_backup_batch_kernel(char* ws, int n, int S, int K, int16_t* pend,
                                                                 const double* prior, const float* value,
                                                                 PuctNoise nz) {
    const int g = blockIdx.x;
    if (g >= n) return;
    const int lane = lane_id();
    PuctTree t = tree_of(ws, g, S);
    const int j0 = t.h->pending;
    if (j0 >= 0) {
        store_pending_eval(t, j0, ws, nz, prior, value, (size_t)g * K);
        return;
    }
    int16_t* pd = pend + (size_t)g * K;
    for (int k = 0; k < K; k++) {
        const int j = pd[k];
        if (j >= 0 && j <= S) store_eval(t, j, prior, value, (size_t)g * K + k);
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

// The visit row that leaves the search (GZ_PUCT_FORCED_PLAYOUTS, gz_forced.h): out = v, and at
// a live root with the full budget every child but the most-visited one (first maximum: c*)
// gives back the forced playouts it would not hold by PUCT against c*'s score.  cfg: c_puct,
// forced_k, S.  The move choice and the tree keep the raw counts.  Every lane of the wave calls.
__device__ inline void prune_row(const PuctTree& t, const PuctHdr* h, const PuctCfg& cfg, const int v[4], int out[4]) {
    const int lane = lane_id();
#pragma unroll
    for (int k = 0; k < 4; k++) out[k] = v[k];
    if (!(cfg.forced_k > 0.0) || h->budget != cfg.S) return;
    // (only an empty cell has a child, and only a child has visits)
    int bv = 0, bi = INT_MAX;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (v[k] > bv) {
            bv = v[k];
            bi = lane + WAVE * k;
        }
    wave_argmax_int(bv, bi);
    if (bv <= 0 || bi >= GZ_CELLS) return;
    const int N = t.visits[0];
    const double sq = __builtin_sqrt((double)N);
    double best = 0.0;
    if ((bi & (WAVE - 1)) == lane) best = forced_score(cfg.c_puct, t.prior[bi], sq, t.W[t.child[bi]] / (double)bv, bv);
    best = __shfl(best, bi & (WAVE - 1));
#pragma unroll 1
    for (int k = 0; k < 4; k++) {  // (one copy of the loop; the result goes to out[k] by select)
        const int c = lane + WAVE * k;
        int n = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) n = j == k ? v[j] : n;
        int kept = n;
        if (c < GZ_CELLS && c != bi && n >= 1)
            kept = forced_kept(n, forced_prune_count(cfg.c_puct, cfg.forced_k, t.prior[c], sq, N - 1, t.W[t.child[c]], n, best));
#pragma unroll
        for (int j = 0; j < 4; j++) out[j] = j == k ? kept : out[j];
    }
}

// FORCED: the row stored is the pruned one
template <bool FORCED>
__device__ inline void finish_game(char* ws, int n, int S, int32_t* moves, int32_t* visits, double* root_q,
                                   gz_search_stats* stats) {
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
        if constexpr (FORCED) {
            int out[4];
            prune_row(t, h, cfg, v, out);  // (a root that is over: v is 0 everywhere and stays)
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (lane + WAVE * k < GZ_CELLS) visits[(size_t)g * GZ_CELLS + lane + WAVE * k] = out[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++)
                if (lane + WAVE * k < GZ_CELLS) visits[(size_t)g * GZ_CELLS + lane + WAVE * k] = v[k];
        }
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

__global__ __launch_bounds__(WAVE) void puct_finish_kernel(char* ws, int n, int S, int32_t* moves, int32_t* visits,
                                                           double* root_q, gz_search_stats* stats) {
    finish_game<false>(ws, n, S, moves, visits, root_q, stats);
}

// puct_finish_kernel of a workspace whose search forces playouts
__global__ __launch_bounds__(WAVE) void puct_finish_forced_kernel(char* ws, int n, int S, int32_t* moves,
                                                                  int32_t* visits, double* root_q,
                                                                  gz_search_stats* stats) {
    finish_game<true>(ws, n, S, moves, visits, root_q, stats);
}

// ---------------------------------------------------------------- Gumbel root (GZ_PUCT_GUMBEL, gz_gumbel.h)
// The ok cells of this lane (bit k: cell lane + 64 k) of a root with the empty cells E and the
// stored row `prior`: the empty cells whose prior has a logarithm, or, when the row has none
// (any_ok false), every empty cell.  Every lane of the wave calls.
__device__ inline int gumbel_ok_cells(const BB& E, const double* prior, bool& any_ok) {
    const int lane = lane_id();
    int emp = 0, okm = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = lane + WAVE * k;
        if (c < GZ_CELLS && bb_test(E, cell_to_bit(c))) {
            emp |= 1 << k;
            if (gumbel_prior_ok(prior[c])) okm |= 1 << k;
        }
    }
    any_ok = ballot(okm != 0) != 0;
    return any_ok ? okm : emp;
}

__device__ inline int wave_max_int(int v) {
    int id = 0;
    wave_argmax_int(v, id);
    return v;
}

// sum of x over the lanes of `mask` in ascending lane order, on top of acc (one running fp64
// sum, as the restatement's); mask is uniform
__device__ inline double wave_running_sum(double acc, double x, uint64_t mask) {
    while (mask) {
        const int l = (int)__builtin_ctzll(mask);
        mask &= mask - 1;
        acc += __shfl(x, l);
    }
    return acc;
}

// Root preparation, once per root, right after node 0's row is stored (each lane reads the
// cells it has just written): the considered cells by m rounds of wave_argmax over
// base = g + logit, gs[c] = base at them and -infinity at every other cell.
__device__ inline void gumbel_root(const PuctTree& t, uint64_t seed, int max_considered, double gumbel_scale,
                                   double* gs) {
    const PuctHdr* h = t.h;
    const int lane = lane_id();
    BB black, white;
    load_bb(black, h->black);
    load_bb(white, h->white);
    bool any_ok;
    const int okm = gumbel_ok_cells(empties(black, white), t.prior, any_ok);
    const uint64_t key = stream_key(seed, h->game_id, h->n_moves, GZ_GUMBEL_SIM);
    double base[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = lane + WAVE * k;
        base[k] = 0.0;
        if ((okm >> k) & 1) base[k] = gumbel_noise(key, c, gumbel_scale) + gumbel_logit(t.prior[c], any_ok);
        if (c < GZ_CELLS) gs[c] = -__builtin_inf();
    }
    const int n_ok = (int)wave_sum_ll(__builtin_popcount(okm));
    const int m = max_considered < n_ok ? max_considered : n_ok;
    int left = okm;
    for (int r = 0; r < m; r++) {
        double bv = -__builtin_inf();
        int bi = INT_MAX;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (((left >> k) & 1) && base[k] > bv) {
                bv = base[k];
                bi = lane + WAVE * k;
            }
        wave_argmax(bv, bi);
        if (bi >= GZ_CELLS) break;  // (base is finite: never)
        if ((bi & (WAVE - 1)) == lane) {
            left &= ~(1 << (bi / WAVE));
            gs[bi] = bv;
        }
    }
}

// The root's cell of simulation t = visits[0] - 1 by the halving schedule: the considered cell
// whose child has seq(m, S)[t] visits and the best gs + sigma(q); -1 without a candidate.
__device__ inline int gumbel_root_cell(const PuctTree& t, const double* gs, const int16_t* seq, int max_considered,
                                       double c_visit, double c_scale, int S) {
    const int lane = lane_id();
    double g[4], w[4];
    int v[4], cons = 0, maxN = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int c = lane + WAVE * k;
        g[k] = -__builtin_inf();
        w[k] = 0.0;
        v[k] = 0;
        if (c < GZ_CELLS) {
            g[k] = gs[c];
            const int cj = t.child[c];
            if (cj >= 0) {
                v[k] = t.visits[cj];
                w[k] = t.W[cj];
            }
        }
        if (g[k] > -__builtin_inf()) cons |= 1 << k;
        if (v[k] > maxN) maxN = v[k];
    }
    const int m = (int)wave_sum_ll(__builtin_popcount(cons));
    maxN = wave_max_int(maxN);
    const int tt = t.visits[0] - 1;
    if (m < 1 || m > max_considered || tt < 0 || tt >= S) return -1;
    const int want = seq[(size_t)(m - 1) * S + tt];
    double bv = -__builtin_inf();
    int bi = INT_MAX;
#pragma unroll
    for (int k = 0; k < 4; k++)
        if (((cons >> k) & 1) && v[k] == want) {
            const double sc = gumbel_score(g[k], c_visit, c_scale, maxN, want, w[k], v[k]);
            if (sc > bv) {
                bv = sc;
                bi = lane + WAVE * k;
            }
        }
    wave_argmax(bv, bi);
    return bi < GZ_CELLS ? bi : -1;
}

// gz_puct_begin with GZ_PUCT_GUMBEL: the tables seq(m', S), m' = 1 .. max_considered
__global__ void puct_gumbel_tables_kernel(int16_t* seq, int max_considered, int S) {
    const int m = blockIdx.x * blockDim.x + threadIdx.x + 1;
    if (m > max_considered) return;
    gumbel_sequence(m, S, seq + (size_t)(m - 1) * S);
}

// puct_select_kernel of a workspace whose search has the Gumbel root
__global__ __launch_bounds__(WAVE) void puct_select_gumbel_kernel(char* ws, int n, int S, uint32_t* leaves,
                                                                  int32_t* active, PuctGumbel gm) {
    const int g = blockIdx.x;
    if (g >= n) return;
    const double c_puct = ((const PuctCfg*)ws)->c_puct;
    const PuctTree t = tree_of(ws, g, S);
    PuctHdr* h = t.h;
    BB black, white;
    load_bb(black, h->black);
    load_bb(white, h->white);
    bool live = false;
    if (!(h->over || h->pending >= 0 || t.visits[0] > h->budget)) {
        const int cell = gumbel_root_cell(t, gm.gs + (size_t)g * GZ_CELLS, gm.seq, gm.max_considered, gm.c_visit,
                                          gm.c_scale, S);
        if (cell >= 0) {
            const Descent d = descend_once<false, false, true>(t, c_puct, S, nullptr, 0, black, white, h->player,
                                                               h->n_moves, 0.0, cell);
            live = d.what == DESCENT_LEAF;
            if (live && lane_id() == 0) h->pending = d.j;
        }
    }
    write_leaf(leaves, active, g, black, white, live);
}

// puct_backup_kernel of such a workspace: the root preparation when node 0 is the pending one
__global__ __launch_bounds__(WAVE) void puct_backup_gumbel_kernel(char* ws, int n, int S, const double* prior,
                                                                  const float* value, PuctGumbel gm) {
    const int g = blockIdx.x;
    if (g >= n) return;
    PuctTree t = tree_of(ws, g, S);
    const int j = t.h->pending;
    if (j < 0) return;
    store_eval(t, j, prior, value, g);
    if (j == 0) gumbel_root(t, gm.seed, gm.max_considered, gm.gumbel_scale, gm.gs + (size_t)g * GZ_CELLS);
    if (lane_id() == 0) t.h->pending = -1;
}

// puct_finish_kernel of such a workspace: the move among the most-visited considered cells by
// gs + sigma(q), no draw; the row is the improved policy softmax(logit + sigma(completed q))
// over the ok cells, scaled to GZ_GUMBEL_ROW_SCALE.  A root that is over: move -1, the zero row.
__global__ __launch_bounds__(WAVE) void puct_finish_gumbel_kernel(char* ws, int n, int S, int32_t* moves,
                                                                  int32_t* visits, double* root_q,
                                                                  gz_search_stats* stats, PuctGumbel gm) {
    const int g = blockIdx.x;
    if (g >= n) return;
    const int lane = lane_id();
    PuctTree t = tree_of(ws, g, S);
    PuctHdr* h = t.h;
    BB black, white;
    load_bb(black, h->black);
    load_bb(white, h->white);
    const bool over = h->over != 0;
    int v[4], out[4] = {0, 0, 0, 0};
    const int sumN = (int)root_visits(t, over, v);
    int mv = -1;
    // (a live root that was never backed up has no row and no gs yet: move -1, the zero row)
    if (!over && t.visits[0] > 0) {
        const double* gs = gm.gs + (size_t)g * GZ_CELLS;
        double w[4], q[4], gv[4], pr[4];
        int maxN = 0, cmax = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const int c = lane + WAVE * k;
            w[k] = v[k] > 0 ? t.W[t.child[c]] : 0.0;
            q[k] = v[k] > 0 ? w[k] / (double)v[k] : 0.0;
            gv[k] = c < GZ_CELLS ? gs[c] : -__builtin_inf();
            pr[k] = c < GZ_CELLS ? t.prior[c] : 0.0;
            if (v[k] > maxN) maxN = v[k];
            if (gv[k] > -__builtin_inf() && v[k] > cmax) cmax = v[k];
        }
        maxN = wave_max_int(maxN);
        cmax = wave_max_int(cmax);
        double bv = -__builtin_inf();
        int bi = INT_MAX;
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (gv[k] > -__builtin_inf() && v[k] == cmax) {
                const double sc = gumbel_score(gv[k], gm.c_visit, gm.c_scale, maxN, cmax, w[k], v[k]);
                if (sc > bv) {
                    bv = sc;
                    bi = lane + WAVE * k;
                }
            }
        wave_argmax(bv, bi);
        mv = bi < GZ_CELLS ? bi : -1;
        if (visits) {
            bool any_ok;
            const int okm = gumbel_ok_cells(empties(black, white), t.prior, any_ok);
            double P = 0.0, A = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                const uint64_t vis = ballot(v[k] > 0);
                P = wave_running_sum(P, pr[k], vis);
                A = wave_running_sum(A, pr[k] * q[k], vis);
            }
            const double v_mix = gumbel_vmix((double)t.value[0], sumN, P, A);
            double x[4], mx = -__builtin_inf();
            int mi = INT_MAX;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                x[k] = 0.0;
                if ((okm >> k) & 1) {
                    x[k] = gumbel_logit(pr[k], any_ok) + gumbel_sigma(gm.c_visit, gm.c_scale, maxN, v[k] > 0 ? q[k] : v_mix);
                    if (x[k] > mx) {
                        mx = x[k];
                        mi = lane + WAVE * k;
                    }
                }
            }
            wave_argmax(mx, mi);
            double Z = 0.0;
#pragma unroll
            for (int k = 0; k < 4; k++) {
                x[k] = ((okm >> k) & 1) ? gz_exp(x[k] - mx) : 0.0;
                Z = wave_running_sum(Z, x[k], ballot((okm >> k) & 1));
            }
#pragma unroll
            for (int k = 0; k < 4; k++)
                if ((okm >> k) & 1) out[k] = gumbel_row_entry(x[k] / Z);
        }
    }
    if (visits) {
#pragma unroll
        for (int k = 0; k < 4; k++)
            if (lane + WAVE * k < GZ_CELLS) visits[(size_t)g * GZ_CELLS + lane + WAVE * k] = out[k];
    }
    if (lane == 0) {
        moves[g] = mv;
        if (root_q) root_q[g] = (over || t.visits[0] == 0) ? 0.0 : -t.W[0] / (double)t.visits[0];
        h->move = mv;
        h->main_draws = 0;
        if (stats) stats[g] = search_stats(over ? 0 : h->n_nodes, h->n_evals, 0, 0);
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
        begin_root(t, black, white, gid, cnt, 3 - mover, over, reuse, budget_of(cap, full, S), full);
        live = !over;
        __threadfence_block();
    }
    write_leaf(leaves, active, g, black, white, live);
    if (remaining && threadIdx.x == 0) {
        const int r = h->over ? 0 : h->budget + 1 - t.visits[0];  // (thread 0 wrote the budget itself)
        remaining[g] = r < 0 ? 0 : r;
    }
}

// Round step 1: a slot whose search is at its budget (B + 1 root visits or more) picks
// its move (wave 0), stashes the visit row of the ply and hands move and statistics to
// selfplay_commit_kernel
// (move -1 leaves the slot alone); then the workgroup re-roots the tree under the move,
// unless the move ends the game -- the tree of a move that ends it no longer matches
// its slot after the commit, and puct_round_kernel begins a fresh one.
// FORCED: the row stashed is the pruned one (prune_row with forced_k).
template <bool FORCED>
__device__ inline void advance_slot(const char* slots, int n, gz_puct_params p, PuctNoise nz, PuctCap cap, char* ws,
                                    int32_t* moves, gz_search_stats* stats, uint16_t* pend, double forced_k) {
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
            if constexpr (FORCED) {
                cfg.forced_k = forced_k;
                int out[4];
                prune_row(t, h, cfg, v, out);
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (lane + WAVE * k < GZ_CELLS) row[lane + WAVE * k] = (uint16_t)out[k];
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++)
                    if (lane + WAVE * k < GZ_CELLS) row[lane + WAVE * k] = (uint16_t)v[k];
            }
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

__global__ __launch_bounds__(RR_THREADS) void puct_advance_kernel(const char* slots, int n, gz_puct_params p,
                                                                  PuctNoise nz, PuctCap cap, char* ws, int32_t* moves,
                                                                  gz_search_stats* stats, uint16_t* pend) {
    advance_slot<false>(slots, n, p, nz, cap, ws, moves, stats, pend, 0.0);
}

// puct_advance_kernel of a run that forces playouts
__global__ __launch_bounds__(RR_THREADS) void puct_advance_forced_kernel(const char* slots, int n, gz_puct_params p,
                                                                         PuctNoise nz, PuctCap cap, char* ws,
                                                                         int32_t* moves, gz_search_stats* stats,
                                                                         uint16_t* pend, double forced_k) {
    advance_slot<true>(slots, n, p, nz, cap, ws, moves, stats, pend, forced_k);
}

// Round step 3: a tree that is not the slot's (a new game, a reset, a move that ended
// the game) gives way to a fresh root, whose board is its leaf of this round; every
// other slot descends once.  (puct_round_forced_kernel below is this kernel with
// descend<true>: a change here belongs there too.)
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
        begin_root(t, black, white, sh->game_id, sh->n_moves, sh->player, false, REUSE_MAGIC,
                   budget_of(cap, full, S), full);
        write_leaf(leaves, active, s, black, white, true);
    }
    if (lane_id() == 0) h->rounds = rounds + 1;
}

// puct_round_kernel of a run that forces playouts: the same step with descend<true>.  (A
// kernel of its own text, not a shared body: routed through a common inline function the
// flag-clear kernel above allocates its registers differently.)
__global__ __launch_bounds__(WAVE) void puct_round_forced_kernel(const char* slots, int n, gz_puct_params p,
                                                                 PuctCap cap, char* ws, uint32_t* leaves,
                                                                 int32_t* active, double forced_k) {
    const int s = blockIdx.x;
    if (s >= n) return;
    const int S = p.num_simulations;
    const SlotHeader* sh = slot_of(slots, s);
    PuctTree t = tree_of(ws, s, S);
    PuctHdr* h = t.h;
    BB black, white;
    load_bb(black, sh->black);
    load_bb(white, sh->white);
    if (sh->game_id >= sh->game_id_end) {
        write_leaf(leaves, active, s, black, white, false);
        return;
    }
    const int rounds = h->reuse == REUSE_MAGIC ? h->rounds : 0;
    if (tree_matches(h, sh)) {
        descend<true>(t, p.c_puct, S, s, leaves, active, forced_k);
    } else {
        const bool full = root_is_full(cap, p.seed, sh->game_id, sh->n_moves);
        begin_root(t, black, white, sh->game_id, sh->n_moves, sh->player, false, REUSE_MAGIC,
                   budget_of(cap, full, S), full);
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
    // W .. board: 4-byte words on both sides
    const uint32_t* a = (const uint32_t*)(src + sizeof(PuctHdr));
    uint32_t* b = (uint32_t*)(dst + 16);
    for (size_t w = threadIdx.x; w < EXPORT_HEAD_BYTES / 4 * M; w += 256) b[w] = a[w];
    // parent, move, term: after the child table
    const char* c = src + sizeof(PuctHdr) + EXPORT_TAIL_OFFSET * M;
    char* d = dst + 16 + EXPORT_HEAD_BYTES * M;
    for (size_t w = threadIdx.x; w < EXPORT_TAIL_BYTES * M; w += 256) d[w] = c[w];
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

// Which workspaces hold a batched search, and which a search that forces playouts.
// gz_puct_select, gz_puct_backup, gz_puct_finish and gz_puct_reroot take no params, and the
// kernel to launch (and its grid of rows) cannot be chosen from the PuctCfg in device memory
// without reading it back, which would synchronise the plain step API too.  So gz_puct_begin
// notes K and the forcing on the host as well, by workspace address; a later plain begin on
// the same address removes the note.
constexpr int NOTE_FORCED = 1 << 16;  // (K <= GZ_PUCT_MAX_LEAVES lies below)
std::mutex g_note_mutex;
std::unordered_map<const void*, int> g_notes;

void note_search(const void* ws, int K, bool forced) {
    std::lock_guard<std::mutex> lock(g_note_mutex);
    if (K > 0 || forced) g_notes[ws] = K | (forced ? NOTE_FORCED : 0);
    else if (!g_notes.empty()) g_notes.erase(ws);
}

int note_of(const void* ws) {
    std::lock_guard<std::mutex> lock(g_note_mutex);
    if (g_notes.empty()) return 0;
    const auto it = g_notes.find(ws);
    return it == g_notes.end() ? 0 : it->second;
}

int leaves_of(const void* ws) { return note_of(ws) & (NOTE_FORCED - 1); }

// the workspaces begun with GZ_PUCT_GUMBEL, and their parameters and region (as the notes above)
std::unordered_map<const void*, PuctGumbel> g_gumbel;

void note_gumbel(const void* ws, const PuctGumbel& gm) {
    std::lock_guard<std::mutex> lock(g_note_mutex);
    if (gm.on) g_gumbel[ws] = gm;
    else if (!g_gumbel.empty()) g_gumbel.erase(ws);
}

bool gumbel_of(const void* ws, PuctGumbel& gm) {
    std::lock_guard<std::mutex> lock(g_note_mutex);
    if (g_gumbel.empty()) return false;
    const auto it = g_gumbel.find(ws);
    if (it == g_gumbel.end()) return false;
    gm = it->second;
    return true;
}

bool forced_of(const void* ws) { return (note_of(ws) & NOTE_FORCED) != 0; }

}  // namespace

// ---------------------------------------------------------------- the host steps the match borrows
namespace gz {

int gz_internal_puct_backup(void* ws, int32_t n, int32_t S, const double* d_prior, const float* d_value,
                            const PuctNoise& nz, void* stream) {
    // (no note is read here: the own-clock rounds and the match come this way without a
    // gz_puct_begin of their own, and a note left by an earlier search on the address is not theirs)
    puct_backup_kernel<<<n, WAVE, 0, as_stream(stream)>>>((char*)ws, n, S, d_prior, d_value, nz);
    return gz_check_launch("puct_backup_kernel");
}

int gz_internal_puct_finish(void* ws, int32_t n, int32_t S, int32_t* d_moves, int32_t* d_visits, double* d_root_q,
                            gz_search_stats* d_stats, void* stream) {
    PuctGumbel gm;
    if (gumbel_of(ws, gm)) {
        puct_finish_gumbel_kernel<<<n, WAVE, 0, as_stream(stream)>>>((char*)ws, n, S, d_moves, d_visits, d_root_q,
                                                                     d_stats, gm);
        return gz_check_launch("puct_finish_gumbel_kernel");
    }
    if (forced_of(ws)) {
        puct_finish_forced_kernel<<<n, WAVE, 0, as_stream(stream)>>>((char*)ws, n, S, d_moves, d_visits, d_root_q,
                                                                     d_stats);
        return gz_check_launch("puct_finish_forced_kernel");
    }
    puct_finish_kernel<<<n, WAVE, 0, as_stream(stream)>>>((char*)ws, n, S, d_moves, d_visits, d_root_q, d_stats);
    return gz_check_launch("puct_finish_kernel");
}

int gz_internal_puct_begin(const gz_board_state* d_boards, const int64_t* d_game_ids, int32_t n_cap, int32_t n,
                           const gz_puct_params* p, void* d_workspace, uint32_t* d_leaves, int32_t* d_active,
                           void* stream) {
    if (!p) return gz_fail(GZ_ERR_ARG, "gz_puct_begin: params is NULL");
    int rc = check_S("gz_puct_begin", n, p->num_simulations);
    if (rc) return rc;
    PuctGumbel gm;
    rc = read_gumbel("gz_puct_begin", p, gm);
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
    double forced_k;
    rc = read_forced("gz_puct_begin", p, forced_k);
    if (rc) return rc;
    if (n > 0 && (!d_boards || !d_game_ids || !d_workspace || !d_leaves || !d_active))
        return gz_fail(GZ_ERR_ARG, "gz_puct_begin: bad arguments");
    if (n == 0) return GZ_OK;
    note_search(d_workspace, K, forced_k > 0.0);
    if (gm.on) gumbel_region(gm, p, d_workspace, n_cap);
    note_gumbel(d_workspace, gm);
    int16_t* pend = K > 0 ? (int16_t*)((char*)d_workspace + rounds_offset(n_cap, p->num_simulations)) : nullptr;
    puct_begin_kernel<<<n, WAVE, 0, as_stream(stream)>>>(d_boards, d_game_ids, n, *p, nz, cap, K, pend,
                                                         (char*)d_workspace, d_leaves, d_active);
    rc = gz_check_launch("puct_begin_kernel");
    if (rc) return rc;
    if (gm.on) {
        // (every begin, so every lock-step ply, writes the tables again: one small launch beside
        // the S+1 forwards, and no state to keep about what a workspace already holds)
        puct_gumbel_tables_kernel<<<1, WAVE, 0, as_stream(stream)>>>(gm.seq, gm.max_considered, p->num_simulations);
        return gz_check_launch("puct_gumbel_tables_kernel");
    }
    if (!(forced_k > 0.0)) return rc;
    puct_forced_cfg_kernel<<<1, 1, 0, as_stream(stream)>>>((char*)d_workspace, forced_k);
    return gz_check_launch("puct_forced_cfg_kernel");
}

int gz_internal_puct_stash_commit(void* d_slots, int32_t n, const SelfplayWs& w, gz_record* d_records,
                                  int32_t record_cap, uint16_t* d_visits, gz_selfplay_counters* d_counters,
                                  void* stream) {
    puct_stash_kernel<<<n, WAVE, 0, as_stream(stream)>>>(w.boards, w.moves, w.visits, n, w.pend);
    int rc = gz_check_launch("puct_stash_kernel");
    if (rc) return rc;
    return gz_internal_selfplay_commit(d_slots, n, w.moves, w.stats, d_records, record_cap, d_counters, w.pend,
                                       d_visits, stream);
}

}  // namespace gz

namespace {

// The backup step of a search whose Gumbel root, if any, the caller names: gm.on with gs set
// (search_impl from its params, gz_puct_backup from the note of its gz_puct_begin).
int backup_step(void* ws, int32_t n, int32_t S, const double* d_prior, const float* d_value, const PuctNoise& nz,
                const PuctGumbel& gm, void* stream) {
    if (!gm.on) return gz_internal_puct_backup(ws, n, S, d_prior, d_value, nz, stream);
    puct_backup_gumbel_kernel<<<n, WAVE, 0, as_stream(stream)>>>((char*)ws, n, S, d_prior, d_value, gm);
    return gz_check_launch("puct_backup_gumbel_kernel");
}

// reroot()'s LDS: map and list, int16 [S+1] each
size_t remap_bytes(int32_t S) { return (4 * ((size_t)S + 1) + 15) & ~(size_t)15; }

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

// One evaluation of a round's rows: the leaf rows turned (GZ_PUCT_LEAF_SYM), the forward,
// the prior rows turned back.
int eval_rows(const LeafSym& ls, const float* d_pv_weights, const RoundBufs& r, int32_t rows, int32_t precision,
              void* stream) {
    int rc = sym_leaves(ls, r.leaves, rows, stream);
    if (rc) return rc;
    rc = gz_pv_forward(d_pv_weights, r.leaves, rows, nullptr, r.logits, r.value, r.probs, r.prior, r.pvws, precision,
                       stream);
    if (rc) return rc;
    return sym_priors(ls, r.prior, rows, stream);
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
    rc = gz_internal_puct_begin(d_boards, d_game_ids, n_cap, n, p, ws, r.leaves, r.active, stream);
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
            rc = eval_rows(ls, d_pv_weights, r, n * K, p->precision, stream);
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
    return gz_internal_puct_finish(ws, n, S, d_moves, d_visits, d_root_q, d_stats, stream);
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
    PuctGumbel gm;
    rc = read_gumbel("gz_puct_search", p, gm);
    if (rc) return rc;
    if (gm.on) gumbel_region(gm, p, ws, n_cap);
    rc = gz_internal_puct_begin(d_boards, d_game_ids, n_cap, n, p, ws, r.leaves, r.active, stream);
    if (rc) return rc;
    for (int round = 0; round <= S; round++) {
        if (round > 0) {
            rc = gz_puct_select(ws, n, S, r.leaves, r.active, stream);
            if (rc) return rc;
        }
        rc = eval_rows(ls, d_pv_weights, r, n, p->precision, stream);
        if (rc) return rc;
        rc = backup_step(ws, n, S, r.prior, r.value, nz, gm, stream);
        if (rc) return rc;
    }
    return gz_internal_puct_finish(ws, n, S, d_moves, d_visits, d_root_q, d_stats, stream);
}

int check_search_args(const char* who, const gz_puct_params* p, int32_t n) {
    if (!p) return gz_fail(GZ_ERR_ARG, std::string(who) + ": params is NULL");
    int rc = check_S(who, n, p->num_simulations);
    if (rc) return rc;
    if (!known_precision(p->precision)) return gz_fail(GZ_ERR_ARG, std::string(who) + ": unknown precision");
    PuctGumbel gm;
    rc = read_gumbel(who, p, gm);
    if (rc) return rc;
    PuctNoise nz;
    rc = read_noise(who, p, nz);
    if (rc) return rc;
    int K;
    rc = read_leaves(who, p, K);
    if (rc) return rc;
    PuctCap cap;
    rc = read_cap(who, p, cap);
    if (rc) return rc;
    double forced_k;
    rc = read_forced(who, p, forced_k);
    if (rc) return rc;
    return check_rows(who, n, K);
}

// gz_selfplay_puct_run(_active): n_slots sized and carved the workspace, the first n plays
int run_impl(const char* who, void* d_slots, int32_t n_slots, int32_t n, const gz_puct_params* p,
             const float* d_pv_weights, void* d_workspace, int32_t n_plies, gz_record* d_records, int32_t record_cap,
             uint16_t* d_visits, gz_selfplay_counters* d_counters, void* stream) {
    int rc = check_search_args(who, p, n_slots);
    if (rc) return rc;
    rc = check_selfplay_args(who, d_slots, n_slots, n_plies, d_counters, d_records, record_cap, d_workspace,
                             d_pv_weights != nullptr, d_visits);
    if (rc) return rc;
    rc = check_active(who, n, n_slots);
    if (rc) return rc;
    const SelfplayWs w = carve_selfplay(d_workspace, n_slots);
    for (int it = 0; it < n_plies; it++) {
        rc = gz_selfplay_boards(d_slots, n, p->num_simulations, w.boards, w.gids, stream);
        if (rc) return rc;
        rc = search_impl(w.boards, w.gids, n_slots, n, p, d_pv_weights, w.puct, w.moves, w.visits, w.root_q, w.stats,
                         stream);
        if (rc) return rc;
        rc = gz_internal_puct_stash_commit(d_slots, n, w, d_records, record_cap, d_visits, d_counters, stream);
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
    if (p->flags & GZ_PUCT_GUMBEL)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": the Gumbel root with tree reuse is not supported");
    rc = check_selfplay_args(who, d_slots, n_slots, n_rounds, d_counters, d_records, record_cap, d_workspace,
                             d_pv_weights != nullptr, d_visits);
    if (rc) return rc;
    int K;
    rc = read_leaves(who, p, K);
    if (rc) return rc;
    if (K > 1)
        return gz_fail(GZ_ERR_ARG, std::string(who) + ": tree reuse with leaves_per_round > 1 is not supported");
    rc = check_active(who, n, n_slots);
    if (rc) return rc;
    const int S = p->num_simulations;
    const SelfplayWs w = carve_selfplay(d_workspace, n_slots);
    // (the trees of these rounds are begun by puct_round_kernel, not by gz_puct_begin: whatever an
    // earlier search noted for this address is over)
    note_gumbel(w.puct, PuctGumbel{});
    const RoundBufs r = carve_rounds(w.puct, n_slots, S);
    const LeafSym ls = leaf_sym(p, w.puct, gz_puct_workspace_bytes(n_slots, S));
    hipStream_t st = as_stream(stream);
    PuctNoise nz;
    rc = read_noise(who, p, nz);
    if (rc) return rc;
    PuctCap cap;
    rc = read_cap(who, p, cap);
    if (rc) return rc;
    double forced_k;
    rc = read_forced(who, p, forced_k);
    if (rc) return rc;
    const bool forced = forced_k > 0.0;
    for (int it = 0; it < n_rounds; it++) {
        if (forced)
            puct_advance_forced_kernel<<<n, RR_THREADS, remap_bytes(S), st>>>(
                (const char*)d_slots, n, *p, nz, cap, (char*)w.puct, w.moves, w.stats, w.pend, forced_k);
        else
            puct_advance_kernel<<<n, RR_THREADS, remap_bytes(S), st>>>((const char*)d_slots, n, *p, nz, cap,
                                                                       (char*)w.puct, w.moves, w.stats, w.pend);
        rc = gz_check_launch(forced ? "puct_advance_forced_kernel" : "puct_advance_kernel");
        if (rc) return rc;
        rc = gz_internal_selfplay_commit(d_slots, n, w.moves, w.stats, d_records, record_cap, d_counters, w.pend,
                                         d_visits, stream);
        if (rc) return rc;
        if (forced)
            puct_round_forced_kernel<<<n, WAVE, 0, st>>>((const char*)d_slots, n, *p, cap, (char*)w.puct, r.leaves,
                                                         r.active, forced_k);
        else
            puct_round_kernel<<<n, WAVE, 0, st>>>((const char*)d_slots, n, *p, cap, (char*)w.puct, r.leaves, r.active);
        rc = gz_check_launch(forced ? "puct_round_forced_kernel" : "puct_round_kernel");
        if (rc) return rc;
        rc = eval_rows(ls, d_pv_weights, r, n, p->precision, stream);
        if (rc) return rc;
        rc = gz_internal_puct_backup(w.puct, n, S, r.prior, r.value, nz, stream);
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
    return rounds_offset(n, S) + rows_bytes((size_t)n);
}

int gz_puct_begin(const gz_board_state* d_boards, const int64_t* d_game_ids, int32_t n, const gz_puct_params* p,
                  void* d_workspace, uint32_t* d_leaves, int32_t* d_active, void* stream) {
    return gz_internal_puct_begin(d_boards, d_game_ids, n, n, p, d_workspace, d_leaves, d_active, stream);
}

int gz_puct_select(void* d_workspace, int32_t n, int32_t S, uint32_t* d_leaves, int32_t* d_active, void* stream) {
    int rc = check_S("gz_puct_select", n, S);
    if (rc) return rc;
    if (n > 0 && (!d_workspace || !d_leaves || !d_active)) return gz_fail(GZ_ERR_ARG, "gz_puct_select: bad arguments");
    if (n == 0) return GZ_OK;
    const int K = leaves_of(d_workspace);
    if (K > 0) return select_batch_impl(d_workspace, n, n, S, K, d_leaves, d_active, stream);
    PuctGumbel gm;
    if (gumbel_of(d_workspace, gm)) {
        puct_select_gumbel_kernel<<<n, WAVE, 0, as_stream(stream)>>>((char*)d_workspace, n, S, d_leaves, d_active, gm);
        return gz_check_launch("puct_select_gumbel_kernel");
    }
    if (forced_of(d_workspace)) {
        puct_select_forced_kernel<<<n, WAVE, 0, as_stream(stream)>>>((char*)d_workspace, n, S, d_leaves, d_active);
        return gz_check_launch("puct_select_forced_kernel");
    }
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
    PuctGumbel gm;
    if (!gumbel_of(d_workspace, gm)) gm = PuctGumbel{};
    return backup_step(d_workspace, n, S, d_prior, d_value, nz, gm, stream);
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
    return rounds_offset(n, S) + batch_pend_bytes(n, K) + 256 + rows_bytes((size_t)n * K);
}

int gz_puct_finish(void* d_workspace, int32_t n, int32_t S, int32_t* d_moves, int32_t* d_visits, double* d_root_q,
                   void* stream) {
    int rc = check_S("gz_puct_finish", n, S);
    if (rc) return rc;
    if (n > 0 && (!d_workspace || !d_moves)) return gz_fail(GZ_ERR_ARG, "gz_puct_finish: bad arguments");
    if (n == 0) return GZ_OK;
    return gz_internal_puct_finish(d_workspace, n, S, d_moves, d_visits, d_root_q, nullptr, stream);
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
    return selfplay_head_bytes(n_slots) + gz_puct_workspace_bytes(n_slots, S);
}

size_t gz_selfplay_puct_batch_workspace_bytes(int32_t n_slots, int32_t S, int32_t K) {
    if (n_slots < 1) n_slots = 1;
    return selfplay_head_bytes(n_slots) + gz_puct_batch_workspace_bytes(n_slots, S, K);
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
    PuctGumbel gm;
    if (gumbel_of(d_workspace, gm))
        return gz_fail(GZ_ERR_ARG, "gz_puct_reroot: tree reuse with the Gumbel root is not supported");
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
    out[0] = part_offset(SELFPLAY_WIDTH, n_slots, SELFPLAY_PARTS - 1);  // pend, the last part
    out[1] = selfplay_head_bytes(n_slots);
    out[2] = out[1] + 256;
    out[3] = game_stride_for(S);
    return GZ_OK;
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

int gz_puct_forced_prune_host(double c_puct, double forced_k, int32_t root_visits, const double prior[225],
                              const double W[225], const int32_t visits[225], int32_t out[225]) {
    if (!forced_k_ok(forced_k)) return gz_fail(GZ_ERR_ARG, "gz_puct_forced_prune_host: forced_k must be finite and in [0, 16]");
    if (root_visits < 1 || !prior || !W || !visits || !out || out == visits)
        return gz_fail(GZ_ERR_ARG, "gz_puct_forced_prune_host: bad arguments");
    for (int c = 0; c < GZ_CELLS; c++)
        if (visits[c] < 0) return gz_fail(GZ_ERR_ARG, "gz_puct_forced_prune_host: a negative visit count");
    forced_prune_row(c_puct, forced_k, root_visits, prior, W, visits, out, GZ_CELLS);
    return GZ_OK;
}

size_t gz_puct_gumbel_bytes(int32_t n, int32_t S, int32_t max_considered) {
    if (n < 1) n = 1;
    if (S < 1) S = 1;
    if (max_considered < 1) max_considered = 1;
    if (max_considered > GZ_GUMBEL_MAX_CONSIDERED) max_considered = GZ_GUMBEL_MAX_CONSIDERED;
    return gumbel_gs_bytes(n) + al256((size_t)max_considered * S * sizeof(int16_t));
}

int gz_puct_gumbel_sequence_host(int32_t m, int32_t S, int16_t* out) {
    if (m < 1 || m > GZ_GUMBEL_MAX_CONSIDERED || S < 1 || S > GZ_MAX_SIMULATIONS || !out)
        return gz_fail(GZ_ERR_ARG, "gz_puct_gumbel_sequence_host: bad arguments");
    gumbel_sequence(m, S, out);
    return GZ_OK;
}

int gz_puct_gumbel_root_host(uint64_t seed, int64_t game_id, int32_t ply, const double prior[225],
                             const uint8_t* empty225, int32_t max_considered, double gumbel_scale,
                             double gs_out[225]) {
    if (!gumbel_args_ok(max_considered, 0.0, 0.0, gumbel_scale))
        return gz_fail(GZ_ERR_ARG, "gz_puct_gumbel_root_host: max_considered must be in [1, 32], gumbel_scale in [0, 8]");
    if (!prior || !empty225 || !gs_out) return gz_fail(GZ_ERR_ARG, "gz_puct_gumbel_root_host: bad arguments");
    gumbel_root_row(stream_key(seed, game_id, ply, GZ_GUMBEL_SIM), prior, empty225, max_considered, gumbel_scale,
                    gs_out);
    return GZ_OK;
}

int gz_puct_gumbel_policy_host(const double prior[225], const double W[225], const int32_t visits[225], double v0,
                               double c_visit, double c_scale, double pi_out[225], int32_t row_out[225]) {
    if (!gumbel_args_ok(1, c_visit, c_scale, 0.0))
        return gz_fail(GZ_ERR_ARG, "gz_puct_gumbel_policy_host: c_visit must be in [0, 1e4], c_scale in [0, 1e3]");
    if (!prior || !W || !visits) return gz_fail(GZ_ERR_ARG, "gz_puct_gumbel_policy_host: bad arguments");
    for (int c = 0; c < GZ_CELLS; c++)
        if (visits[c] < 0) return gz_fail(GZ_ERR_ARG, "gz_puct_gumbel_policy_host: a negative visit count");
    gumbel_policy_row(prior, nullptr, W, visits, v0, c_visit, c_scale, pi_out, row_out);
    return GZ_OK;
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
