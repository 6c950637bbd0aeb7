/*
 * gzero.h -- C-ABI of libgzero.so, the MI355X (gfx950) self-play engine that
 * replaces the hot path of gitMasterLiujiahui/AlphaZero-Gomoku.
 *
 * The reference is pure Python with no FFI, so every entry point below
 * replaces a Python call site; the binding a maintainer would add (ctypes,
 * the same shape as cgo/JNI) is in INTEGRATION.md and in
 * alphazero-gomoku_amd/gzero/_lib.py.
 *
 * Conventions
 *  - All pointers named d_* are DEVICE pointers owned by the caller (torch
 *    tensors in the Python host).  `stream` is a hipStream_t passed as void*.
 *    Calls are stream-ordered and asynchronous; none allocates or synchronises.
 *  - Return value: GZ_OK (0) or a negative GZ_ERR_*; gz_last_error() holds a
 *    thread-local message.  Misuse (bad sizes) is rejected before any launch.
 *  - Boards are bit planes: row r in word r>>1, bits (r&1)*16 + c (c < 15);
 *    bit 15 of each row and row 15 are zero.  Cells are row-major r*15+c.
 */
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GZ_OK 0
#define GZ_ERR_ARG -1
#define GZ_ERR_HIP -2
#define GZ_ERR_UNSUPPORTED -3
#define GZ_ERR_INTERNAL -4

#define GZ_MAX_SIMULATIONS 4095
#define GZ_MAX_GAME_PLIES 200

/* GomokuBoard state (gomoku_board.py:40-53): stones, len(move_history),
 * current_player (1/2), game_over, winner (0 = None). 80 bytes. */
typedef struct gz_board_state {
    uint32_t black[8];
    uint32_t white[8];
    int32_t n_moves;
    int32_t player;
    int32_t over;
    int32_t winner;
} gz_board_state;

/* AlphaZeroGomokuAI search knobs (ai_agent.py:29-31,65-90); difficulty maps
 * to num_simulations / c_puct / exploration exactly as the reference's table. */
typedef struct gz_search_params {
    int32_t num_simulations; /* params["num_simulations"] */
    int32_t max_depth;       /* rollout cap, _simulate max_depth (100) */
    double c_puct;           /* params["c_puct"] */
    double exploration;      /* params["exploration"] */
    double beta;             /* constructor beta: weight of tanh(pattern/1e4) in UCB */
    uint64_t seed;           /* RNG streams (gzero/rng.py) */
    int32_t planner_steps;   /* BG-planner plies per rollout (> 0: gz_plan_search / gz_selfplay_plan_run) */
    int32_t flags;           /* GZ_FLAG_* */
} gz_search_params;

#define GZ_FLAG_GATHER_LEAVES 1 /* append every non-terminal node's board for the PV forward */
#define GZ_FLAG_GN_CHECK 2      /* planner searches: also run the full GraphNet forward on every
                                   incremental row and count differing rows (gz_plan_gn_stats) */

/* BGPlannerAI.params (bg_planner.py:215-219): easy {8, 0.5, 0.2}, medium
 * {12, 0.65, 0.1}, hard {16, 0.75, 0.05}. */
typedef struct gz_planner_params {
    int32_t k;       /* knowledge-search top-k, 1..16 */
    int32_t pad;
    double alpha;    /* mix_alpha */
    double explore;  /* exploration probability */
} gz_planner_params;

/* One (s, pi, z) training tuple (training.py:77-97,203-210). 80 bytes. */
typedef struct gz_record {
    uint32_t black[8]; /* planes before the move (absolute colours) */
    uint32_t white[8];
    int64_t game_id;
    int16_t ply;    /* move number within the game */
    int16_t move;   /* r*15+c */
    int8_t player;  /* mover, 1/2 */
    int8_t z;       /* +1 mover won, -1 lost, 0 draw */
    int8_t pad[2];
} gz_record;

typedef struct gz_search_stats {
    int32_t n_nodes;
    int32_t predicts;   /* GomokuModel.predict calls the reference makes for this move */
    int32_t main_draws; /* draws on the (game, ply, 0) stream */
    int32_t pad;
    int64_t sim_draws;  /* draws summed over simulation streams */
} gz_search_stats;

typedef struct gz_selfplay_counters {
    int32_t records;         /* records written to d_records */
    int32_t leaves;          /* boards the searches produced: the first min(leaves, leaf_cap) are
                                in d_leaves, the counter goes on counting past leaf_cap */
    int32_t records_dropped; /* records lost because d_records was full */
    int32_t leaves_dropped;  /* never written (stays as the caller set it): a full leaf buffer
                                shows as leaves > leaf_cap, and the leaves - leaf_cap rows past
                                the end were dropped.  Do not add this field to that difference. */
    int64_t moves;           /* plies played */
    int64_t games;           /* games finished */
    int64_t mcts_moves;      /* plies decided by MCTS (n_moves >= 6; the opening plies
                                0-5 of _opening_move do no search, ai_agent.py:138-166) */
} gz_selfplay_counters;

const char* gz_last_error(void);
int gz_version(void);

/* ---- K1: board step / legal mask / five-in-a-row (gomoku_board.py:84-213) ----
 * d_boards[i] <- make_move(d_moves[i]) (cell r*15+c, or any value outside
 * [0,225) which fails like an off-board move).  d_ok[i] = make_move's return.
 * d_legal (optional) = [n][4] uint64 row-major masks of empty cells after the
 * step (get_valid_moves, which ignores game_over). */
int gz_board_step(gz_board_state* d_boards, const int32_t* d_moves, int32_t n, int32_t* d_ok,
                  uint64_t* d_legal, void* stream);

/* ---- rollout policy and rollouts (ai_agent.py:251-430) ----
 * Component entry points used by the parity tests. keys = RNG stream keys. */
int gz_policy_move(const gz_board_state* d_boards, const uint64_t* d_keys, int32_t n, int32_t* d_moves,
                   uint32_t* d_draws, void* stream);
int gz_rollout(const gz_board_state* d_boards, const int32_t* d_ai, const uint64_t* d_keys, int32_t n,
               int32_t max_depth, double* d_values, gz_board_state* d_final, uint32_t* d_draws,
               void* stream);

/* ---- pattern score / _bg_score (bg_planner.py:133-196, ai_agent.py:432-439) ---- */
int gz_pattern_score(const gz_board_state* d_boards, const int32_t* d_player, int32_t n, int64_t* d_score,
                     double* d_bg, void* stream);

/* ---- K2+K3: one AlphaZeroGomokuAI.get_move per board (ai_agent.py:109-222) ----
 * One wavefront per board.  d_trees: n * gz_tree_bytes(num_simulations)
 * scratch holding each search tree (layout in DESIGN.md; readable by tests: entries
 * [0, n_nodes) of every array are the tree, the entries past them are undefined).
 * d_moves[i] = chosen cell or -1 (None).  Leaves are appended to d_leaves
 * ([leaf_cap][16] uint32: black[8], white[8]) when GZ_FLAG_GATHER_LEAVES.
 * *d_leaf_count (the caller zeroes it) is advanced by every leaf produced, also
 * past leaf_cap: rows at or past leaf_cap are not written, so a full buffer shows
 * as *d_leaf_count > leaf_cap and the excess rows were dropped (no separate
 * dropped-leaves count is kept: gz_selfplay_counters.leaves_dropped is never written). */
size_t gz_tree_bytes(int32_t num_simulations);
int gz_search(const gz_board_state* d_boards, const int64_t* d_game_ids, int32_t n,
              const gz_search_params* p, void* d_trees, int32_t* d_moves, gz_search_stats* d_stats,
              uint32_t* d_leaves, int32_t leaf_cap, int32_t* d_leaf_count, void* stream);

/* ---- self-play collector (training.py:141-218) over n_slots concurrent games ----
 * Slot s plays games game_id_base + s + g*game_id_stride, g = 0,1,2,...  Each
 * call advances every slot by n_plies plies; a finished game's tuples (with z)
 * are appended to d_records and the slot restarts from the empty board.
 * d_leaf_meta (optional, [leaf_cap] int32) tags every gathered leaf for
 * gz_pv_forward_tree: -1 = a search root, i >= 0 = a child of the node at leaf
 * index i (one stone more; that node is the root or one of its children), -2 =
 * any deeper node.
 * Memory contract.  d_slots needs no initialisation: gz_selfplay_init writes the whole
 * 128-byte header of every slot; the record area behind it is written ply by ply before
 * it is read.  d_counters is added to, never cleared: the caller zeroes it (before the
 * first call, or before every call for per-call counts; leaves_dropped is never written).
 * d_records, d_visits (PUCT entries), d_leaves and d_leaf_meta are written at the rows the
 * counters count and nowhere else: rows at or past min(records, record_cap), or
 * min(leaves, leaf_cap), keep what they held.  Every byte of a written record is
 * defined (pad is 0). */
size_t gz_slot_bytes(int32_t num_simulations);
int gz_selfplay_init(void* d_slots, int32_t n_slots, int32_t num_simulations, int64_t game_id_base,
                     int64_t game_id_stride, void* stream);
int gz_selfplay_run(void* d_slots, int32_t n_slots, const gz_search_params* p, int32_t n_plies,
                    gz_record* d_records, int32_t record_cap, uint32_t* d_leaves, int32_t leaf_cap,
                    int32_t* d_leaf_meta, gz_selfplay_counters* d_counters, void* stream);
/* gz_selfplay_run with BG-planner rollout plies (p->planner_steps > 0): each ply
 * is one gz_plan_search over all slots (host-driven, synchronises the stream
 * once per simulation round) followed by the same record / restart logic;
 * d_leaf_meta (optional) as for gz_selfplay_run.
 * d_workspace: gz_selfplay_plan_workspace_bytes(n_slots, num_simulations). */
size_t gz_selfplay_plan_workspace_bytes(int32_t n_slots, int32_t num_simulations);
int gz_selfplay_plan_run(void* d_slots, int32_t n_slots, const gz_search_params* p, const gz_planner_params* pp,
                         const float* d_gn_weights, void* d_workspace, int32_t n_plies, gz_record* d_records,
                         int32_t record_cap, uint32_t* d_leaves, int32_t leaf_cap, int32_t* d_leaf_meta,
                         gz_selfplay_counters* d_counters, void* stream);
/* per slot, totals over every search it ran since gz_selfplay_init: d_out[3s] =
 * predict() calls, d_out[3s+1] = main-stream RNG draws, d_out[3s+2] = simulation-
 * stream draws (the checker's view of rollout / planner decisions, ai_agent.py:168-285) */
int gz_selfplay_draws(const void* d_slots, int32_t n_slots, int64_t* d_out, void* stream);
/* A bounded game range (training.py:374-377 plays exactly its n games per iteration):
 * a slot whose next game id would be >= game_id_end goes idle instead of restarting --
 * gz_selfplay_run / gz_selfplay_plan_run skip it and record nothing for it (default:
 * no end, continuous refill). */
int gz_selfplay_set_game_end(void* d_slots, int32_t n_slots, int64_t game_id_end, void* stream);
/* Copies the slots into d_dst (another n_slots-slot buffer) with the active ones first
 * and the idle ones after, each in slot order; *d_n_active = the active count.  A slot
 * holds its whole game state, so the caller may then run the first *d_n_active slots
 * of d_dst only.  d_workspace: gz_selfplay_compact_workspace_bytes(n_slots). */
size_t gz_selfplay_compact_workspace_bytes(int32_t n_slots);
int gz_selfplay_compact(const void* d_slots, int32_t n_slots, void* d_dst, int32_t* d_n_active, void* d_workspace,
                        void* stream);
/* current board of every slot (for inspection / tests) */
int gz_selfplay_boards(const void* d_slots, int32_t n_slots, int32_t num_simulations,
                       gz_board_state* d_out, int64_t* d_game_ids, void* stream);

/* ---- K6: AlphaZeroGomokuNet forward (neural_network.py:94-159,214-252) ----
 * d_weights: packed blob of gz_pv_weight_floats() floats (layout in
 * csrc/gz_pvnet.h / gzero/weights.py).  Boards [n][16] uint32 bit planes.  If
 * d_count is not NULL it holds the number of valid boards on the device
 * (n = capacity; output rows at or past min(*d_count, n) are not written and keep what
 * they held).  The workspace needs no initialisation, here and in every other entry point
 * that takes one, unless its comment says otherwise (gz_selfplay_puct_reset, the GraphNet
 * statistics).  Outputs: logits [n][225], value [n] (tanh), probs
 * [n][225] (softmax) or NULL; prior (optional, needs probs) = [n][225] float64
 * MCTSNode._get_prior_probability (ai_agent.py:564-582): the softmax at the empty
 * cells renormalised by their float64 sum (numpy's pairwise order), 0 at stones --
 * the reference's compact vector is prior[i][empty cells, row-major].
 * precision: GZ_PV_FP32 (exact f32 MFMA) or
 * GZ_PV_F16X3 (3-term fp16 split on the fp16 MFMA, ~22-bit operands, f32
 * accumulation) or GZ_PV_F16 (below).  d_workspace: gz_pv_workspace_bytes(n)
 * bytes, required (fp32: per-wave slabs; f16x3 and f16: the 1x1 head convs' outputs
 * of every board, 2,816 B each, passed from the tower kernel to the batched FC-heads
 * kernel). */
#define GZ_PV_FP32 0
#define GZ_PV_F16X3 1
/* GZ_PV_F16: the f16x3 forward with the lo terms of the residual tower dropped, one
 * fp16 MFMA per product where f16x3 issues three.  conv0 as in f16x3 (0/1 inputs,
 * w_hi + w_lo, fp32 BN, ReLU), its output stored as fp16(x0).  Each residual conv:
 * acc = sum fp16(w) * a in an f32 accumulator (k order: tap, then 4 x 32 channels), a
 * the stored fp16 activation; y = relu(fma(acc, S, T) (+ skip)) in fp32, S / T the
 * blob's fp32 BN affine, skip the block input as stored; y1, x1, y2 stored as
 * fp16(y).  The last epilogue feeds the 1x1 head convs from its fp32 y (x2 is never
 * rounded); heads, softmax, value and prior are f16x3's kernels.  Batch-invariant like
 * f16x3; same workspace.  Opt-in (the PUCT search): its logits differ from the fp32
 * forward's by ~1e-4 at init weights, more at trained magnitudes. */
#define GZ_PV_F16 2
size_t gz_pv_weight_floats(void);
size_t gz_pv_workspace_bytes(int32_t n);
int gz_pv_forward(const float* d_weights, const uint32_t* d_boards, int32_t n, const int32_t* d_count,
                  float* d_logits, float* d_value, float* d_probs, double* d_prior, void* d_workspace,
                  int32_t precision, void* stream);

/* The forward under a board symmetry.  t = 2 k + f, k in 0..3 rotations, f in {0, 1}:
 * y = flip^f(rot90^k(x)) -- np.rot90 (counter-clockwise), then np.flip along the columns,
 * both colour planes together (training.py's _transform_planes) -- and a 225-wide row o_y
 * computed on y goes back to x's frame as np.rot90(np.flip(o_y, 1) if f else o_y, -k);
 * t = 0 is the identity.  gz_pv_sym: d_sym [n] uint8 = the transform of every row, a pure
 * function of the seed and the row's 16 words (gzero/rng.py's mix64 / draw):
 *   key = mix64(seed + GOLDEN); for i in 0..7: key = mix64(key ^ (row[i] | row[8+i] << 32))
 *   t   = draw(key, 0x53594D4D) >> 61
 * gz_pv_sym_host: one row by the same code on the host, no GPU, 0..7.
 * gz_pv_forward_sym is gz_pv_forward of the transformed boards with every non-NULL
 * 225-wide output (logits, probs, prior) mapped back and the value as it is: the prior is
 * the row gz_pv_forward gives for y (renormalised in y's cell order), permuted, not a prior
 * recomputed in x's order.  d_sym not NULL: row i uses d_sym[i] & 7 and the seed is not
 * read; d_sym NULL: row i uses gz_pv_sym's t.  d_boards is not modified; rows at or past
 * min(*d_count, n) are not written.  d_workspace: gz_pv_sym_workspace_bytes(n) =
 * gz_pv_workspace_bytes(n), the transformed boards (64 n) and one byte per row, each
 * rounded up to 256.  Argument errors as gz_pv_forward, before any launch. */
int gz_pv_sym(const uint32_t* d_boards, int32_t n, uint64_t seed, uint8_t* d_sym, void* stream);
int gz_pv_sym_host(uint64_t seed, const uint32_t row[16]);
size_t gz_pv_sym_workspace_bytes(int32_t n);
int gz_pv_forward_sym(const float* d_weights, const uint32_t* d_boards, int32_t n, const int32_t* d_count,
                      const uint8_t* d_sym, uint64_t seed, float* d_logits, float* d_value, float* d_probs,
                      double* d_prior, void* d_workspace, int32_t precision, void* stream);

/* Incremental forward of the nodes of MCTS searches (MCTSNode.__init__ ->
 * GomokuModel.predict, ai_agent.py:522-523; neural_network.py:132-159), f16x3:
 * d_meta as written by gz_selfplay_run.  Roots and untagged nodes run the full
 * forward (roots also keep their intermediate maps and pre-BN accumulators, at
 * most root_cap of them) and are bit-identical to gz_pv_forward(..., GZ_PV_F16X3,
 * ...) of the same boards.  A root's children are the root's pre-BN accumulators
 * plus the convolution of their one-stone input differences (radius 1..4 per
 * layer's input): the same network in f16x3 arithmetic with fp32 accumulation in
 * another order, within 2e-5 of the full forward's logits / value (1e-4 of the
 * reference's fp32 forward).  The children of a root child (grandchildren) are
 * the same delta taken from their parent: the parent's pre-ReLU values (its
 * patch, fp32, inside the squares its stone changed; the root's elsewhere) plus
 * the convolution of the grandchild's one-stone differences -- a delta of a
 * delta, under the same 2e-5 / 1e-4 bounds, not the full forward's values given
 * the patch (the patches of 145,920 B share one pool of 1,736,704 B per root map
 * slot, 11.9 patches each; the grandchildren of parents beyond it take the full
 * forward, so give root_cap room where roots have a dozen such parents).  A tag whose
 * board does not differ from its parent's by exactly one cell is ignored (full
 * forward), so the tags only decide speed.  d_workspace:
 * gz_pv_tree_workspace_bytes(n, root_cap) bytes (~2.4 MB per root: the x0 map
 * 128 KB, pre-ReLU values 512 KB, the patch pool 1.7 MB).  It has no precision argument:
 * the tree forward is f16x3 only (there is no GZ_PV_F16 tree forward). */
size_t gz_pv_tree_workspace_bytes(int32_t n, int32_t root_cap);
int gz_pv_forward_tree(const float* d_weights, const uint32_t* d_boards, const int32_t* d_meta, int32_t n,
                       const int32_t* d_count, int32_t root_cap, float* d_logits, float* d_value, float* d_probs,
                       double* d_prior, void* d_workspace, void* stream);
/* d_out6 (device int32[6]) = the last tree forward's list sizes: roots seen, roots
 * with stored maps, incremental children, full-forward boards, incremental
 * grandchildren, parents that claimed a patch slot. */
int gz_pv_tree_stats(const void* d_workspace, int32_t n, int32_t* d_out6, void* stream);
/* d_out2 (device int32[2]) = the 16-row x 128-channel x 1152-deep MFMA tiles of the
 * residual convs the last tree forward's incremental kernels executed, for root
 * children and for grandchildren (measurement: bench.py's executed-FLOP roofline). */
int gz_pv_tree_exec_tiles(const void* d_workspace, int32_t n, int32_t* d_out2, void* stream);

/* ---- K7: BG planner nets (bg_planner.py:22-78, BGPlannerAI.get_move :243-250) ----
 * d_weights: packed blob of gz_gn_weight_floats() floats (csrc/gz_gnet.h,
 * gzero/planner_nets.py).  Boards [n][16] uint32 bit planes (d_count as above).
 * Outputs: p = softmax(GraphNet(planes)) [n][225], q = OpponentDQN(planes)
 * [n][225], logits [n][225] or NULL.  GraphNet convs in f16x3 (as GZ_PV_F16X3);
 * the policy FC and the DQN run batched over 32 boards per workgroup (fp32 MFMA);
 * a launch of fewer than 64 boards per CU without logits runs them split over output
 * tiles instead (16 boards x 4 tiles per workgroup, three launches, p and q the same
 * bits), the layers' outputs through the workspace.  GZ_GN_SMALL_HEADS=<rows> moves
 * that threshold (A/B knob).
 * d_workspace: gz_gn_workspace_bytes(n) bytes, required (per row a 3.6 KB net record,
 * then 3 KB of the split heads' scratch). */
size_t gz_gn_weight_floats(void);
size_t gz_gn_workspace_bytes(int32_t n);
int gz_gn_forward(const float* d_weights, const uint32_t* d_boards, int32_t n, const int32_t* d_count,
                  float* d_p, float* d_q, float* d_logits, void* d_workspace, void* stream);

/* ---- K4+K5+K7: MCTS with BG-planner rollout plies (planner_steps > 0) ----
 * gz_search's contract (ai_agent.py:109-222) for p->planner_steps >= 0 with the
 * planner of pp (BGPlannerAI for the searching AI's colour, bg_planner.py:199-269)
 * and its nets d_gn_weights (gz_gn_forward).  Host-driven: launches on `stream`
 * and synchronises it once per simulation round.  d_workspace:
 * gz_plan_workspace_bytes(n, num_simulations) bytes.  d_trees (optional) gets
 * gz_tree_bytes(num_simulations) bytes per game in gz_search's layout.
 * Footprint (C = max(n, 65536) GN rows per planner step, capped at n*S): per game
 * its context + tree and S 128-B jobs; per row 0.9 KB of p / q, a 6.6 KB net
 * workspace (gz_gn_workspace_bytes(1)) and, always reserved, the same again for
 * GZ_FLAG_GN_CHECK's full-forward copy (0.56 GB each at C = 65536); and n + C
 * incremental-GraphNet map slots of 232 KB (16.2 GB at n = 4096, S = 200 -- 17.4 GB
 * in all). */
size_t gz_plan_workspace_bytes(int32_t n, int32_t num_simulations);
int gz_plan_search(const gz_board_state* d_boards, const int64_t* d_game_ids, int32_t n,
                   const gz_search_params* p, const gz_planner_params* pp, const float* d_gn_weights,
                   void* d_workspace, void* d_trees, int32_t* d_moves, gz_search_stats* d_stats,
                   uint32_t* d_leaves, int32_t leaf_cap, int32_t* d_leaf_count, void* stream);

/* Incremental planner nets inside gz_plan_search / gz_selfplay_plan_run: a planner
 * ply's board is its predecessor plus the planner's move, and a rollout's first
 * board usually the search root plus one stone (bg_planner.py:243-250,
 * ai_agent.py:251-285), so GraphNet recomputes only the radius 1..5 squares around
 * the new stone from kept maps (the root's, or the rollout's own chain); the outputs
 * are bit-identical to gz_gn_forward's.  GZ_GN_INC=0 in the environment turns it
 * off.  out[4] (host) = rows run by the full forward, by the incremental forward,
 * rows checked against the full forward (GZ_FLAG_GN_CHECK) and rows that differed,
 * summed since the last reset (reset != 0 zeroes them after reading; the counters
 * start undefined until the first reset).  gz_selfplay_plan_gn_stats takes
 * gz_selfplay_plan_run's workspace. */
/* The incremental GraphNet on explicit chains (tests, tools): row i's 32-byte tag
 * (csrc/gz_gnet.h GnTag) = {mode, base, job, cell, nst, stones[6], pad}: mode 0 =
 * full forward, its maps and policy-conv outputs kept in slot `job`; mode 1 = the
 * board is the board of slot `base` plus the stone `cell`, with the squares of the
 * earlier stones stones[0..nst) (added since `base`) in slot `job`, where this row's
 * squares go too.  Slots: gz_gn_slot_bytes() each.  p, q as gz_gn_forward (bit-
 * identical).  Rows of one call must use distinct `job` slots, and no row's `job`
 * may be another row's `base`.  d_workspace: gz_gn_chain_workspace_bytes(n). */
size_t gz_gn_slot_bytes(void);
size_t gz_gn_chain_workspace_bytes(int32_t n);
int gz_gn_forward_chain(const float* d_weights, const uint32_t* d_boards, int32_t n, const void* d_tags,
                        void* d_slots, float* d_p, float* d_q, void* d_workspace, void* stream);
int gz_plan_gn_stats(void* d_workspace, int32_t n, int32_t num_simulations, int64_t* out, int32_t reset,
                     void* stream);
int gz_selfplay_plan_gn_stats(void* d_workspace, int32_t n_slots, int32_t num_simulations, int64_t* out,
                              int32_t reset, void* stream);

/* ---- network-guided PUCT search (opt-in mode; csrc/gz_puct.hip, gz_puct.h) ----
 * The default search reproduces the reference, which never reads the network's
 * outputs.  In this mode the priors steer selection and the value head replaces
 * the rollout: per simulation the tree is descended by
 *   score(c) = q + ((c_puct * prior[c]) * sqrt((double)visits[node])) / (1.0 + n),
 *   q = n ? W[child] / n : 0.0,  first maximum over the empty cells (fp64, that order),
 * a new child is created and evaluated by the network ((double)float32 value v for
 * its side to move) and backup(i, v) runs s = -v; visits[i] += 1; W[i] += s; s = -s
 * up the parents (W is from the view of the player who moved into the node).  A
 * terminal node backs up -1 (a five) or 0 (full board / 200 plies, make_move's
 * rules) on every visit.  The root is evaluated first, so a search of S simulations
 * is S+1 rounds of (select, forward over the n leaf rows, backup) with no host
 * synchronisation; a game with no leaf in a round has the empty board in its row.
 * Move: with n_moves >= temp_plies the empty cell with the most root-child visits
 * (first maximum); else one draw x of the (seed, game, ply, 0) stream and the first
 * cell whose running visit sum exceeds (x * total) >> 64.  No opening book or
 * epsilon-exploration; Dirichlet noise at the root is opt-in (GZ_PUCT_ROOT_NOISE).  A board that is over returns move -1 and zero visits.
 * d_visits (optional) int32 [n][225] root-child visits; d_root_q (optional) the
 * root's mean value for its side to move, -W[0] / visits[0].
 * Workspace layout, node record (~2.3 KB: 1.9 GB at 4096 games x 200 simulations)
 * and the export layout of gz_puct_trees are documented in csrc/gz_puct.h. */
typedef struct gz_puct_params {
    int32_t num_simulations; /* S, 1..GZ_MAX_SIMULATIONS */
    int32_t temp_plies;      /* plies (move counts below this) that sample the move from the visits */
    double c_puct;
    uint64_t seed;           /* RNG streams (gzero/rng.py) */
    int32_t precision;       /* GZ_PV_FP32 / GZ_PV_F16X3 / GZ_PV_F16: the forward of every search and self-play entry */
    int32_t flags;           /* 0 or GZ_PUCT_ROOT_NOISE | GZ_PUCT_LEAF_BATCH | GZ_PUCT_PLAYOUT_CAP | GZ_PUCT_LEAF_SYM |
                                GZ_PUCT_FORCED_PLAYOUTS | GZ_PUCT_GUMBEL */
} gz_puct_params;
/* Dirichlet noise at the search root (opt-in; AlphaZero's exploration in self-play).
 * With GZ_PUCT_ROOT_NOISE in flags the p given to gz_puct_begin, gz_puct_search,
 * gz_selfplay_puct_run and gz_selfplay_puct_rounds points at a gz_puct_noise_params;
 * without it nothing past the 32 bytes of gz_puct_params is read.  The root's stored
 * (and exported) prior row becomes, at its empty cells,
 *   prior'[c] = (1.0 - noise_eps) * prior[c] + noise_eps * eta[c],  eta ~ Dir(noise_alpha),
 * eta[c] = g[c] / total, g[c] a Gamma(noise_alpha) sample that cell c draws from the
 * (seed, game, the root's move count, 0x4E4F4953) stream (draw indices 256 c .. 256 c +
 * 255; csrc/gz_dirichlet.h), total their running fp64 sum in ascending cell order; a
 * total of 0 (or not finite) leaves the row alone.  Exactly once per root: a fresh
 * root (gz_puct_begin's, a move without a child, a new game) when its evaluation is
 * backed up, an inherited root right after the re-root, on its carried row with the
 * key of its new ply; gz_puct_reroot's move -1 mixes nothing.  Other nodes, the visit
 * rows, the move choice and the backup are unchanged, and the sampler is plain fp64
 * arithmetic that rounds identically on the device, the host and in CPython
 * (tests/puct_noise_ref.py).  noise_alpha must be finite and in [1e-3, 1e3],
 * noise_eps in [0, 1] (GZ_ERR_ARG otherwise).  gz_puct_begin keeps the three values in
 * the workspace for gz_puct_backup and gz_puct_reroot, which take no params. */
#define GZ_PUCT_ROOT_NOISE 1
typedef struct gz_puct_noise_params {
    gz_puct_params base;
    double noise_alpha;
    double noise_eps;
} gz_puct_noise_params;      /* 48 bytes */
/* Leaf batching with virtual loss (opt-in): K leaves per game per round, so a move takes
 * about 1 + ceil(S/K) rounds of n K rows instead of S+1 rounds of n -- for small n, where
 * a forward of a few boards leaves the chip idle.  With GZ_PUCT_LEAF_BATCH in flags p
 * points at a gz_puct_batch_params (its noise fields are read only with
 * GZ_PUCT_ROOT_NOISE); without it nothing past the 32 (48) bytes is read and every entry
 * point computes what it did before.  leaves_per_round K in 1..GZ_PUCT_MAX_LEAVES
 * (GZ_ERR_ARG otherwise, before any GPU call).  Round 0 evaluates the root alone (row
 * g K; the game's other rows are inactive).  In every later round a game descends up to
 * K times, one descent after the other, while finished + in-flight simulations
 * (visits[0] + vl[0]) <= S.  vl[x] counts the round's waiting leaves below node x and
 * enters the score as that many visits, each lost by the selector (a node's W is from
 * the selector's view):
 *   n = visits[j] + vl[j],  q = n ? (W[j] - (double)vl[j]) / (double)n : 0.0,
 *   score = q + ((c_puct * prior[c]) * sqrt((double)(visits[i] + vl[i]))) / (1.0 + (double)n)
 * so K = 1 is the unbatched search bit for bit.  A descent that ends in a terminal node
 * backs up at once and takes no row; one that selects a node created in this round and
 * not yet evaluated (a collision) changes nothing and ends the game's selection for the
 * round; any other creates a node, whose board goes to the game's next row.  The backup
 * step stores and backs up the active rows of a game in ascending row order.  vl lives
 * for one select launch only and is never stored.  The first descent of a round cannot
 * collide, so every unfinished game completes at least one simulation per round, a move
 * takes between 1 + ceil(S/K) and S+1 rounds, the root's visit row still sums to S and a
 * tree never exceeds S+1 nodes; a game at its budget has only inactive rows.
 * gz_puct_begin stores K in the workspace (and notes it for that workspace address on the
 * host): gz_puct_select / gz_puct_backup then treat d_leaves, d_active, d_prior and
 * d_value as [n K] rows, game g at rows g K .. g K + K - 1; gz_puct_finish and
 * gz_puct_trees work unchanged.  The workspace is gz_puct_batch_workspace_bytes(n, S, K)
 * (gz_selfplay_puct_batch_workspace_bytes for gz_selfplay_puct_run).  A round of only
 * terminal descents has no active row although the search is not over, so a step-API
 * caller asks gz_puct_remaining: d_remaining [n] = S + 1 - visits[0], 0 when the game is
 * over.  gz_puct_search and gz_selfplay_puct_run run 1 + ceil(S/K) rounds, read the
 * largest remaining count back and run ceil(left/K) more until it is 0: unlike the
 * unbatched search, the batched one synchronises the calling host thread with the stream
 * (one 4-byte read per block of rounds; it cannot be captured into a graph).  Tree reuse
 * with K > 1 is not supported: gz_puct_reroot and gz_selfplay_puct_rounds return
 * GZ_ERR_ARG. */
#define GZ_PUCT_LEAF_BATCH 2
#define GZ_PUCT_MAX_LEAVES 32
typedef struct gz_puct_batch_params {
    gz_puct_noise_params noise;   /* base and, with GZ_PUCT_ROOT_NOISE, the noise */
    int32_t leaves_per_round;     /* K */
    int32_t pad;
} gz_puct_batch_params;      /* 56 bytes */
/* Playout cap randomization (opt-in; KataGo's way to cheaper training games): every ply
 * is independently a full search (S simulations, root noise, a training target) with
 * probability full_prob, or a fast one (F = fast_simulations, no noise, played and not
 * trained on).  With GZ_PUCT_PLAYOUT_CAP in flags p points at a gz_puct_cap_params (its
 * noise fields are read only with GZ_PUCT_ROOT_NOISE, leaves_per_round not at all);
 * without it nothing past the 32 / 48 / 56 bytes is read and every entry point computes
 * what it did before.
 *   full(seed, game, ply) = to_unit(draw(stream_key(seed, game, ply, 0x50434150), 0)) < full_prob
 * (gzero/rng.py; the constant spells "PCAP"): a pure function of (seed, game id, ply), with
 * no counter, independent of the move-sampling stream (..., 0) and of the noise stream.
 * The budget B of the root at ply n_moves is S on a full ply and F on a fast one; it is
 * decided when the node becomes a root (a fresh root: gz_puct_begin, a new game, a move
 * without a child; an inherited one: right after the re-root) and kept with the tree.  A
 * search is finished when its root has B+1 visits or more.  An inherited root may arrive
 * with v >= B+1 visits (a fast ply after a full one whose chosen child was visited more
 * than F times): it gets no simulation -- gz_puct_select gives it an inactive row,
 * gz_selfplay_puct_rounds picks its move in the next round -- and its visit row is the
 * inherited child visits as they are, summing to v-1 >= B; every other row sums to B.  A
 * move takes B+1 rounds on a fresh root and max(1, B+1-v) on an inherited one.  A tree
 * still never exceeds S+1 nodes: workspaces, the tree stride and the export layout are
 * unchanged.  With GZ_PUCT_ROOT_NOISE only the roots of full plies are mixed (at the same
 * two places); a fast root's row is left alone, also one inherited from a full ply (as a
 * child it never was mixed).  gz_puct_remaining and gz_puct_reroot's d_remaining return
 * max(0, B+1-visits[0]); gz_puct_finish and the move choice are unchanged (temp_plies
 * applies to fast plies too).  Accepted by gz_puct_begin (which keeps F and full_prob in
 * the workspace for select, backup and reroot), gz_puct_search, gz_puct_reroot,
 * gz_selfplay_puct_rounds(_active) and gz_selfplay_puct_run(_active) -- the last two are
 * correct but gain nothing: the lock-step engine runs S+1 rounds for everybody, and only
 * the own-clock engine turns a smaller budget into fewer rounds.  GZ_ERR_ARG before any
 * launch: fast_simulations outside [1, S], full_prob not finite or outside [0, 1], the
 * flag together with GZ_PUCT_LEAF_BATCH, the flag in gz_puct_match_run's search params.
 * The record format is unchanged; gz_puct_cap_full tells which records were full plies. */
#define GZ_PUCT_PLAYOUT_CAP 4
typedef struct gz_puct_cap_params {
    gz_puct_batch_params batch;  /* base; the noise fields are read only with GZ_PUCT_ROOT_NOISE */
    int32_t fast_simulations;    /* F, 1..num_simulations */
    int32_t pad;
    double  full_prob;           /* p, finite, in [0, 1] */
} gz_puct_cap_params;            /* 72 bytes */
/* Which plies were full: d_full [n] uint8 = full(seed, d_records[i].game_id,
 * d_records[i].ply) for every record (one thread each; the same seed and full_prob as the
 * run that made them).  gz_puct_cap_full_host: one decision, 0 or 1, by the same code on
 * the host, no GPU. */
int gz_puct_cap_full(const gz_record* d_records, int32_t n, uint64_t seed, double full_prob, uint8_t* d_full,
                     void* stream);
int gz_puct_cap_full_host(uint64_t seed, int64_t game_id, int32_t ply, double full_prob);
/* Forced playouts and policy-target pruning (opt-in; KataGo's paper, section 3.2, the
 * companion of root noise and the playout cap).  With GZ_PUCT_FORCED_PLAYOUTS in flags p
 * points at a gz_puct_forced_params (its inner fields are read only with their own flags);
 * without it nothing past the 32 / 48 / 56 / 72 bytes is read and every entry point computes
 * what it did before.  Everything is fp64 in exactly the order written (csrc/gz_forced.h;
 * tests/puct_forced_ref.py restates it), sqrt and / correctly rounded.
 * Forcing, at the root only and only at a root whose budget is the full one (budget == S:
 * every root without the playout cap, the full plies with it; fast plies neither force nor
 * prune).  T = visits[0] - 1.  For an empty cell c whose child j has n = visits[j] >= 1:
 *   forced(c) = sqrt((forced_k * prior[0][c]) * (double)T)
 *   if ((double)n < forced(c))  score(c) = +infinity      (else the score as it is)
 * prior[0] is the root's stored row (the noised one with GZ_PUCT_ROOT_NOISE); several
 * infinite scores resolve by the first-maximum rule (lowest cell); a terminal child is forced
 * like any other.  Nodes below the root, the backup, the move choice and the budget are
 * unchanged.
 * Pruning, where a root's visit row leaves the search: gz_puct_finish's d_visits (so the row
 * of a lock-step self-play ply) and the row an own-clock ply stashes.  The move is picked
 * from the raw counts and gz_puct_trees exports the raw visits.  With N = visits[0],
 * sq = sqrt((double)N) and the raw counts v[c] of a full-budget root:
 *   c* = the empty cell with the most visits, first maximum; n* = v[c*]  (n* == 0: row unchanged)
 *   best = W[child c*] / n* + ((c_puct * prior[0][c*]) * sq) / (1.0 + (double)n*)
 *   every other cell c with n = v[c] >= 1, q = W[child c] / (double)n held fixed:
 *     m = min(n, (int)forced(c))                   (forced(c) with T = N - 1; truncation)
 *     r = 0;  while r < m:  s = q + ((c_puct * prior[0][c]) * sq) / (1.0 + (double)(n - (r + 1)));
 *                           if s >= best: break;  r += 1
 *     out[c] = n - r;  if r > 0 and out[c] == 1: out[c] = 0
 *   out[c*] = n*
 * A pruned row sums to at most the raw sum and never to 0 while n* > 0 (gz_dataset_pi
 * normalises a row by its own sum).  forced_k = 0 forces nothing and prunes nothing: the flag
 * with k = 0 gives the flag-clear bytes.  A root that is over gives the zero row as before.
 * Accepted by gz_puct_begin (which keeps forced_k with the workspace for gz_puct_select and
 * gz_puct_finish), gz_puct_search, gz_selfplay_puct_run(_active) and
 * gz_selfplay_puct_rounds(_active).  gz_puct_reroot takes no params and reads nothing of
 * this: the workspace stays what gz_puct_begin made it, so the searches after a re-root force
 * and prune as the one before.  Combines with GZ_PUCT_ROOT_NOISE, GZ_PUCT_PLAYOUT_CAP and
 * GZ_PUCT_LEAF_SYM.  GZ_ERR_ARG before any launch: forced_k not finite or outside [0, 16],
 * the flag together with GZ_PUCT_LEAF_BATCH (virtual loss and forcing are not defined
 * together), the flag in gz_puct_match_run's search params (an arena plays, it collects no
 * targets).  Workspace sizes, the tree stride, the record format and the pend / d_visits
 * layouts are unchanged. */
#define GZ_PUCT_FORCED_PLAYOUTS 16
typedef struct gz_puct_forced_params {
    gz_puct_cap_params cap;  /* base; its fields are read only with their own flags */
    double forced_k;         /* KataGo's k (2), finite, in [0, 16] */
} gz_puct_forced_params;     /* 80 bytes */
/* The pruning of one row by the same code on the host, no GPU: visits[c] == 0 means no child
 * at c (W[c] and prior[c] are then not read), root_visits = N >= 1, out != visits. */
int gz_puct_forced_prune_host(double c_puct, double forced_k, int32_t root_visits, const double prior[225],
                              const double W[225], const int32_t visits[225], int32_t out[225]);
/* The Gumbel root with sequential halving (opt-in; "Policy improvement by planning with
 * Gumbel", Danihelka et al., ICLR 2022): a search of S = 16..32 simulations that still
 * improves the policy.  With GZ_PUCT_GUMBEL in flags p points at a gz_puct_gumbel_params (its
 * inner fields are not read: the flag combines with GZ_PUCT_LEAF_SYM only); without it
 * nothing past the bytes read before is read and every entry point computes what it did.
 * Everything is fp64 in exactly the order written (csrc/gz_gumbel.h; tests/puct_gumbel_ref.py
 * restates it), with gz_log / gz_exp of csrc/gz_dirichlet.h.  q lives in [-1, 1], so
 * c_scale = 0.5 is the paper's 1.0 on values in [0, 1]; there is no min-max rescaling.
 * Root preparation, once per root, when node 0's evaluation is stored (the backup step).
 * E = the root's empty cells; a cell of E is ok when DBL_MIN <= prior[0][c] <= DBL_MAX; with
 * no ok cell every cell of E is ok with logit 0.0, else logit(c) = gz_log(prior[0][c]).
 *   u = unit_open(draw(stream_key(seed, game, ply, 0x47554D42), c));  e = -gz_log(u);
 *   if (!(e >= DBL_MIN)) e = 0x1p-53;   g(c) = gumbel_scale * (-gz_log(e));
 *   base(c) = g(c) + logit(c);   m = min(max_considered, ok cells)
 *   considered: m times the first maximum of base over the ok cells not yet taken;
 *   gs[c] = base(c) at the considered cells, -infinity elsewhere.
 * Schedule, seq(m, S), in integers (gz_puct_gumbel_sequence_host):
 *   m <= 1: 0, 1, .., S-1;  else L = ceil(log2 m), visits = [0]*m, k = m, and while fewer
 *   than S entries: x = max(1, S / (L k)); x times: append visits[:k], visits[i] += 1 for
 *   i < k; then k = max(2, k / 2).  The first S entries.
 * Root selection at simulation t = visits[0] - 1: want = seq(m, S)[t]; among the considered
 * cells whose child has want visits (no child: 0), with maxN the largest root-child count,
 *   score(c) = want == 0 ? gs[c] : gs[c] + ((c_visit + (double)maxN) * c_scale) * (W[child] / (double)N)
 * the first maximum (there always is a candidate; without one nothing descends).  Below the
 * root the descent, the backup, the terminal rules and the budget are the search's own: a
 * search is still S+1 rounds.
 * The move: among the considered cells with the most visits the first maximum of
 * gs[c] + sigma(q(c)), sigma(q) = ((c_visit + maxN) * c_scale) * q.  temp_plies is not read
 * and main_draws is 0: the Gumbel draw already samples.  gumbel_scale = 0 is deterministic.
 * The policy target, the row that leaves the search (gz_puct_finish's d_visits, so the row of
 * a lock-step self-play ply): over the visited children N(c), q(c) = W / N, sumN = sum N,
 * P and A the running sums in ascending cell order of prior[c] and prior[c] * q(c),
 *   v0 = (double)value[0];  v_mix = (sumN > 0 && P > 0) ? (v0 + sumN * (A / P)) / (1.0 + sumN) : v0
 *   x(c) = logit(c) + sigma(visited ? q(c) : v_mix) over all ok cells;  mx = max x
 *   e(c) = gz_exp(x(c) - mx);  Z = the running sum in ascending cell order;  pi(c) = e(c) / Z
 *   row[c] = (int32)(pi(c) * 32767.0 + 0.5), 0 at every other cell.
 * 32767 survives the uint16 rows and the int16 views of them; gz_dataset_pi divides a row by
 * its own sum, so the scale cancels; the largest entry is at least 146, so no row is empty.
 * Unchanged: d_root_q, the exported tree (raw visits, the root's stored row), a board that is
 * over (move -1, the zero row).
 * Workspace: the caller allocates the flag-clear size (plus gz_puct_sym_bytes(rows) with
 * GZ_PUCT_LEAF_SYM) rounded up to 256, plus gz_puct_gumbel_bytes(n, S, max_considered): gs
 * f64 [n][225], then the tables seq(m', S), m' = 1..max_considered, int16, which gz_puct_begin
 * writes.  With the flag clear nothing past the flag-clear size is touched.
 * Honoured by gz_puct_begin / select / backup / finish (begin notes the search with the
 * workspace), gz_puct_search and gz_selfplay_puct_run(_active); with every precision.
 * GZ_ERR_ARG before any launch: max_considered outside [1, 32]; c_visit not finite or outside
 * [0, 1e4], c_scale outside [0, 1e3], gumbel_scale outside [0, 8]; the flag together with
 * GZ_PUCT_ROOT_NOISE, GZ_PUCT_LEAF_BATCH, GZ_PUCT_PLAYOUT_CAP or GZ_PUCT_FORCED_PLAYOUTS; the
 * flag in gz_selfplay_puct_rounds(_active) and gz_puct_match_run; gz_puct_reroot on a
 * workspace begun with the flag (an inherited root has no schedule). */
#define GZ_PUCT_GUMBEL 32
#define GZ_PUCT_GUMBEL_MAX_CONSIDERED 32
#define GZ_PUCT_GUMBEL_ROW_SCALE 32767
typedef struct gz_puct_gumbel_params {
    gz_puct_forced_params forced; /* base; none of its inner fields is read */
    int32_t max_considered;       /* 1..32 (16) */
    int32_t pad;
    double c_visit;               /* 50 */
    double c_scale;               /* 0.5 on q in [-1, 1] */
    double gumbel_scale;          /* 1; 0: no noise */
} gz_puct_gumbel_params;          /* 112 bytes */
size_t gz_puct_gumbel_bytes(int32_t n, int32_t num_simulations, int32_t max_considered);
/* The same code on the host, no GPU.  sequence: out[S].  root: empty225[c] != 0 = an empty
 * cell; gs_out[225]; returns GZ_OK.  policy: visits[c] == 0 means no child at c (W[c] is then
 * not read); every cell counts as empty, so a stone carries a prior that is not ok (0.0); pi_out
 * and row_out [225], either may be NULL. */
int gz_puct_gumbel_sequence_host(int32_t m, int32_t num_simulations, int16_t* out);
int gz_puct_gumbel_root_host(uint64_t seed, int64_t game_id, int32_t ply, const double prior[225],
                             const uint8_t* empty225, int32_t max_considered, double gumbel_scale,
                             double gs_out[225]);
int gz_puct_gumbel_policy_host(const double prior[225], const double W[225], const int32_t visits[225], double v0,
                               double c_visit, double c_scale, double pi_out[225], int32_t row_out[225]);
/* Leaf symmetry (opt-in; AlphaGo Zero's random board symmetry per leaf evaluation): with
 * GZ_PUCT_LEAF_SYM in flags every leaf x is evaluated as
 *   t = gz_pv_sym(seed, x);  (prior_y, value) = gz_pv_forward(T_t(x));  prior[c] mapped back
 * (gz_pv_forward_sym below, with d_sym NULL and seed = p->seed, is exactly that), at the
 * search's precision.  No new params struct: the seed is gz_puct_params.seed, and the flag
 * combines with GZ_PUCT_ROOT_NOISE, GZ_PUCT_LEAF_BATCH and GZ_PUCT_PLAYOUT_CAP wherever those
 * combine; without it every entry point computes what it did before.  t is a function of
 * the seed and the position alone -- not of the game, the ply or the row -- so a position
 * met twice is evaluated the same way, tree reuse and compaction carry valid evaluations
 * and the step API's caller needs no state.  Root noise is mixed into the mapped-back row.
 * Honoured by gz_puct_search (also batched), gz_selfplay_puct_run(_active),
 * gz_selfplay_puct_rounds(_active) and gz_puct_match_run (both sides under the same t).
 * The step API (gz_puct_begin / select / backup / reroot / finish) accepts the flag and does
 * nothing with it: there the caller is the evaluator and calls gz_pv_forward_sym itself.
 * Workspace: the *_workspace_bytes functions return what they did; with the flag set the
 * caller allocates that size plus gz_puct_sym_bytes(rows), rows = n K (gz_puct_search) or
 * n_slots K (self-play, the match: K = 1), and the extra region starts at the flag-clear
 * size.  With the flag clear nothing past the flag-clear size is touched. */
#define GZ_PUCT_LEAF_SYM 8
size_t gz_puct_sym_bytes(int32_t rows);
/* includes the forward's workspace and gz_puct_search's leaf / output rows */
size_t gz_puct_workspace_bytes(int32_t n, int32_t num_simulations);
size_t gz_puct_batch_workspace_bytes(int32_t n, int32_t num_simulations, int32_t leaves_per_round);
/* Step API (the caller supplies the evaluator): begin writes the root boards to
 * d_leaves [n][16] and d_active [n] (1 = the row wants an evaluation); after the
 * caller's backup of the roots, S times select (new leaves) and backup; d_prior
 * [n][225] float64 and d_value [n] in gz_pv_forward's layouts, rows of inactive
 * games ignored.  finish picks the moves. */
int gz_puct_begin(const gz_board_state* d_boards, const int64_t* d_game_ids, int32_t n, const gz_puct_params* p,
                  void* d_workspace, uint32_t* d_leaves, int32_t* d_active, void* stream);
int gz_puct_select(void* d_workspace, int32_t n, int32_t num_simulations, uint32_t* d_leaves, int32_t* d_active,
                   void* stream);
int gz_puct_backup(void* d_workspace, int32_t n, int32_t num_simulations, const double* d_prior,
                   const float* d_value, void* stream);
int gz_puct_finish(void* d_workspace, int32_t n, int32_t num_simulations, int32_t* d_moves, int32_t* d_visits,
                   double* d_root_q, void* stream);
/* simulations left to each game's budget (never below 0), 0 when the game is over (any search of this mode) */
int gz_puct_remaining(void* d_workspace, int32_t n, int32_t num_simulations, int32_t* d_remaining, void* stream);
/* begin, the S+1 rounds with gz_pv_forward(d_pv_weights, p->precision), finish */
int gz_puct_search(const gz_board_state* d_boards, const int64_t* d_game_ids, int32_t n, const gz_puct_params* p,
                   const float* d_pv_weights, void* d_workspace, int32_t* d_moves, int32_t* d_visits,
                   double* d_root_q, void* stream);
/* the trees of the last search on this workspace, gz_puct_tree_bytes(S) per game:
 * int32 n_nodes, evaluated nodes, main-stream draws, move; then in creation order
 * W f64[S+1], prior f64[S+1][225], visits i32[S+1], leaf value f32[S+1], board
 * u32[S+1][16], parent i16[S+1], move u8[S+1] (255 = root), term u8[S+1].
 * Entries [0, n_nodes) of every array are the tree; the entries past them are undefined.
 * A node that is never evaluated (a terminal node, the root of a board that is over) has
 * an all-zero prior row and value 0; a node that still waits for its evaluation (between
 * a select, begin or reroot and the backup) has no prior row yet: it is undefined. */
size_t gz_puct_tree_bytes(int32_t num_simulations);
int gz_puct_trees(const void* d_workspace, int32_t n, int32_t num_simulations, void* d_out, void* stream);
/* Self-play with this search (slots as gz_selfplay_init): per ply the slots'
 * boards, gz_puct_search, then the same record / restart logic as gz_selfplay_run.
 * The root visit counts are the policy target: a game's rows wait in the workspace
 * ([n_slots][200][225] uint16) and, when it ends, go to d_visits [record_cap][225]
 * at the indices of its records (dropped with records that overflow).  Slot
 * statistics (gz_selfplay_draws): nodes evaluated, main draws (0 or 1 per ply), 0. */
size_t gz_selfplay_puct_workspace_bytes(int32_t n_slots, int32_t num_simulations);
size_t gz_selfplay_puct_batch_workspace_bytes(int32_t n_slots, int32_t num_simulations, int32_t leaves_per_round);
int gz_selfplay_puct_run(void* d_slots, int32_t n_slots, const gz_puct_params* p, const float* d_pv_weights,
                         void* d_workspace, int32_t n_plies, gz_record* d_records, int32_t record_cap,
                         uint16_t* d_visits, gz_selfplay_counters* d_counters, void* stream);
/* Tree reuse between plies (opt-in; the entry points above are unchanged).  A search
 * is finished when its root has S+1 visits.  After the move m the subtree of the root's
 * child at m is the next ply's tree: its nodes keep their creation order and are
 * renumbered densely, in place; W, visits, prior, value, board and term are carried bit
 * for bit, the new root has parent -1 and move 255, the header's position advances by
 * m.  A root that arrives with v visits needs S+1-v more simulations (at least one).
 * gz_puct_reroot (step API), per game: d_moves[g] = -1 leaves the tree untouched; a
 * move with a child re-roots (a terminal child: the game is over); a move without one
 * gives a fresh one-node root that waits for its evaluation, its board in leaf row g
 * with d_active[g] = 1 (every other case: an empty, inactive row).  d_remaining
 * (optional) int32 [n]: simulations left to the budget, 0 when the game is over.  On a
 * game at its budget gz_puct_select gives an inactive row, so games that inherit
 * different visit counts can share the rounds until the last is done. */
int gz_puct_reroot(void* d_workspace, int32_t n, int32_t num_simulations, const int32_t* d_moves,
                   uint32_t* d_leaves, int32_t* d_active, int32_t* d_remaining, void* stream);
/* Self-play with reuse, every slot on its own clock: n_rounds rounds of (slots at
 * their budget pick and play their move, every slot re-roots / begins a fresh root as
 * needed and descends once, one forward over the n_slots leaf rows, backup), with no
 * host synchronisation and no copy to the host.  Every live slot has one leaf in every
 * forward; a move takes S+1-v rounds.  Records, visit rows (each sums to S), counters
 * as gz_selfplay_puct_run; slot statistics (gz_selfplay_draws), added when a move is
 * played: the rounds in which the slot's leaf was evaluated, main draws, the rounds the
 * move took (S+1 for a fresh root, S+1-v for an inherited one); a game's moves depend only on
 * (seed, game id, weights, params), not on the slots or on how rounds are cut into
 * calls.  Same workspace as gz_selfplay_puct_run.  gz_selfplay_puct_reset marks every
 * tree invalid: required before the first round and after anything else used the
 * workspace (a tree is reused only while its root is the slot's game id and position). */
int gz_selfplay_puct_reset(void* d_workspace, int32_t n_slots, int32_t num_simulations, void* stream);
int gz_selfplay_puct_rounds(void* d_slots, int32_t n_slots, const gz_puct_params* p, const float* d_pv_weights,
                            void* d_workspace, int32_t n_rounds, gz_record* d_records, int32_t record_cap,
                            uint16_t* d_visits, gz_selfplay_counters* d_counters, void* stream);
/* A workspace carved for its capacity and run for its active count.  The two entry
 * points above with one more argument: n_slots is the capacity that sized and carved
 * d_workspace (gz_selfplay_puct_workspace_bytes / gz_selfplay_puct_batch_workspace_bytes
 * of n_slots), so the pending visit rows, the trees and the round buffers keep their
 * places; every kernel grid, the forward's rows (n_active, or n_active K when batched)
 * and the remaining count cover the first n_active slots only, 1 <= n_active <= n_slots.
 * A game's moves and rows do not depend on n_active.  gz_selfplay_puct_run and
 * gz_selfplay_puct_rounds are these with n_active = n_slots. */
int gz_selfplay_puct_run_active(void* d_slots, int32_t n_slots, int32_t n_active, const gz_puct_params* p,
                                const float* d_pv_weights, void* d_workspace, int32_t n_plies, gz_record* d_records,
                                int32_t record_cap, uint16_t* d_visits, gz_selfplay_counters* d_counters,
                                void* stream);
int gz_selfplay_puct_rounds_active(void* d_slots, int32_t n_slots, int32_t n_active, const gz_puct_params* p,
                                   const float* d_pv_weights, void* d_workspace, int32_t n_rounds,
                                   gz_record* d_records, int32_t record_cap, uint16_t* d_visits,
                                   gz_selfplay_counters* d_counters, void* stream);
/* Byte offsets in the self-play workspace of n_slots slots (the same with and without
 * leaf batching; leaves_per_round 0 or 1 = unbatched): out[0] the pending visit rows
 * (uint16 [n_slots][200][225]), out[1] the PUCT block (the d_workspace of gz_puct_trees),
 * out[2] the first tree (out[1] + 256), out[3] the per-game tree stride; the round
 * buffers begin at out[2] + n_slots out[3]. */
int gz_selfplay_puct_layout(int32_t n_slots, int32_t num_simulations, int32_t leaves_per_round, size_t out[4]);
/* Slot compaction of a PUCT engine with a bounded game range (gz_selfplay_set_game_end),
 * in place: among the first n_active slots a are active (game_id < game_id_end); the
 * holes are the idle slots below a, the fillers the active slots at or above a -- equally
 * many -- and the k-th filler goes to the k-th hole, both ascending.  Sources and
 * destinations are disjoint, so the moves run in parallel and nothing needs a second copy
 * of the trees or the pending rows; the order of the slots is NOT preserved (per-slot
 * views such as gz_selfplay_draws and gz_selfplay_boards are permuted with them).
 *   slot buffers      the pair trades places: d_slots stays a permutation of what it was;
 *   pending rows      rows [0, n_moves) of the filler move to the hole's place;
 *   trees             only with move_trees (the tree-reuse engine): the tree header and
 *                     rows [0, n_nodes) of every array, byte for byte, reuse mark included
 *                     (a tree belongs to its slot at the new index exactly when it did at
 *                     the old one).  Lock-step and batched searches rebuild every tree
 *                     each ply and pass move_trees = 0.
 * What the hole held (its old tree and rows) is dead and stays as it is, as does the
 * filler's old place.  The gs rows of a GZ_PUCT_GUMBEL engine (lock-step only) are not
 * moved: they are dead between plies, every ply's root preparation writes its own.
 * d_order [n_active]: the new index of each old slot (the identity except at the pairs);
 * *d_n_active = a; the caller then runs the first a slots
 * (gz_selfplay_puct_run_active / _rounds_active).  No active slot below a, or no idle
 * one: only d_order and d_n_active are written.  d_puct_workspace: the self-play
 * workspace of n_slots slots; d_workspace: gz_selfplay_puct_compact_workspace_bytes(n_slots).
 * GZ_ERR_ARG: n_active outside [1, n_slots], leaves_per_round outside [0, 32], or
 * leaves_per_round > 1 with move_trees; nothing is launched then. */
size_t gz_selfplay_puct_compact_workspace_bytes(int32_t n_slots);
int gz_selfplay_puct_compact(void* d_slots, int32_t n_slots, int32_t n_active, int32_t num_simulations,
                             int32_t leaves_per_round, int32_t move_trees, void* d_puct_workspace,
                             int32_t* d_order, int32_t* d_n_active, void* d_workspace, void* stream);

/* The arena: two networks play each other (gz_selfplay_puct_run_active with the evaluator
 * chosen per game).  The slots are gz_selfplay_init's, bounded with
 * gz_selfplay_set_game_end so that each plays one game and goes idle.  Side A (index 0)
 * and side B (index 1) each bring a weight blob and a precision; A plays black in game g
 * iff ((g ^ a_black_parity) & 1) == 0.  The side that moves at a search's root evaluates
 * every leaf of that search: each player searches with its own network.  Per ply, over
 * the first n_active slots:
 *   boards   gz_selfplay_boards;
 *   plan     one workgroup: side[s] = the mover's side (-1: an idle slot, whose board is
 *            marked over, so it takes no part in the search), row_of[s] = the slot's rank
 *            among the slots of its side in ascending slot order, and the two counts;
 *   rounds   the S+1 rounds of gz_puct_search, the evaluation of each being
 *              gather    leaf row s (64 bytes) -> packed leaves of side[s], row row_of[s];
 *              forward   gz_pv_forward(d_weights[i], packed i, n_active, &count[i], ...,
 *                        precision[i]) for i = 0, 1: the counts stay on the device;
 *              scatter   packed prior row (225 fp64) and value -> slot row s of the round
 *                        buffers, on which select, backup and finish run as they are;
 *   commit   the visit row is stashed and the move played as gz_selfplay_puct_run does:
 *            records, visit rows and counters keep their meaning.
 * Nothing synchronises the host.  search: the shared S, temp_plies, c_puct, seed and
 * flags (0 or GZ_PUCT_ROOT_NOISE, then a gz_puct_noise_params; not GZ_PUCT_PLAYOUT_CAP); search->precision is not
 * read.  A game's moves, visit rows and z depend only on (seed, game id, the two blobs
 * and precisions, the search params, a_black_parity), not on n_slots, n_active, how
 * plies are cut into calls, or compaction.  Workspace (gz_puct_match_workspace_bytes): it
 * begins with the self-play workspace of n_slots slots (gz_selfplay_puct_workspace_bytes),
 * so gz_selfplay_puct_layout and gz_selfplay_puct_compact(..., move_trees = 0, ...) work
 * on it as they are; side and row_of (int32 [n_slots] each), the counts and the two
 * packed buffer sets (leaves, logits, probs, value, prior and the forward's workspace,
 * n_slots rows each) follow.  GZ_ERR_ARG before any launch: a NULL pointer, an unknown
 * precision, a_black_parity outside {0, 1}, n_active outside [1, n_slots],
 * GZ_PUCT_LEAF_BATCH in the flags.  Per-side simulation counts, leaf batching and tree
 * reuse (a subtree holds the other side's evaluations) are not part of a match. */
typedef struct gz_puct_match_params {
    const gz_puct_params* search;
    const float* d_weights[2];     /* side A, side B */
    int32_t precision[2];          /* GZ_PV_FP32 / GZ_PV_F16X3 / GZ_PV_F16 per side */
    int32_t a_black_parity;        /* 0 or 1 */
    int32_t pad;
} gz_puct_match_params;      /* 40 bytes */
size_t gz_puct_match_workspace_bytes(int32_t n_slots, int32_t num_simulations);
int gz_puct_match_run(void* d_slots, int32_t n_slots, int32_t n_active, const gz_puct_match_params* mp,
                      void* d_workspace, int32_t n_plies, gz_record* d_records, int32_t record_cap,
                      uint16_t* d_visits, gz_selfplay_counters* d_counters, void* stream);
/* The score of a match from its records: adds to *d_tally (integer atomics; the caller
 * zeroes it once per match and calls this after every step's records).  A game is
 * counted once, at its ply-0 record (the mover is black, z black's result); plies counts
 * records.  d_result (optional, int8 [n_games]): d_result[game_id - game_id_base] = +1 (A
 * won), -1 (B won) or 0 (a draw); games not in d_records are left alone, ids outside
 * [game_id_base, game_id_base + n_games) are tallied and not written. */
typedef struct gz_puct_match_tally {
    int64_t games, a_wins, b_wins, draws;
    int64_t a_wins_black, a_wins_white, b_wins_black, b_wins_white;
    int64_t plies;
} gz_puct_match_tally;       /* 72 bytes */
int gz_puct_match_results(const gz_record* d_records, int32_t n_records, int32_t a_black_parity,
                          int64_t game_id_base, int32_t n_games, gz_puct_match_tally* d_tally, int8_t* d_result,
                          void* stream);

/* The noise sampler on its own (the device and host functions the search runs).
 * gz_puct_root_noise: d_eta [n][225] = eta at the empty cells of each board (ply =
 * n_moves) and 0 at stones; an all-zero row when the total is 0 or the board is full.
 * gz_puct_root_noise_host: the same code on the host, no GPU (empty225: non-zero =
 * empty cell). */
int gz_puct_root_noise(const gz_board_state* d_boards, const int64_t* d_game_ids, int32_t n, uint64_t seed,
                       double alpha, double* d_eta, void* stream);
int gz_puct_root_noise_host(uint64_t seed, int64_t game_id, int32_t ply, const uint8_t* empty225, double alpha,
                            double* eta225);

/* BGPlannerAI.get_move (bg_planner.py:232-269) for each board: d_ai = the
 * planner's colour P, d_keys = RNG stream; d_moves (-1 = None), d_draws.
 * d_workspace: gz_planner_move_workspace_bytes(n) bytes. */
size_t gz_planner_move_workspace_bytes(int32_t n);

/* KnowledgeSearch.score_move(board, (r, c), player) (bg_planner.py:90-106) for
 * every cell of every board, the side to move playing the stone: d_scores
 * [n][225] float64 -- 1e6 (the move wins for player), -1e5 (player's opponent can
 * then complete five, _opponent_can_win_next :116-125), else _pattern_score +
 * _center_bias (:127-196); -1e9 at occupied cells (is_valid_move fails).
 * top_k_moves (:108-114) = the first k cells of a stable descending sort. */
int gz_knowledge_scores(const gz_board_state* d_boards, const int32_t* d_player, int32_t n, double* d_scores,
                        void* stream);
int gz_planner_move(const gz_board_state* d_boards, const int32_t* d_ai, const uint64_t* d_keys, int32_t n,
                    const gz_planner_params* pp, const float* d_gn_weights, void* d_workspace,
                    int32_t* d_moves, uint32_t* d_draws, void* stream);

/* ---- K8 training-set materialisation (GomokuSelfPlayDataset, training.py:104-134;
 * augment_sample, training.py:44-71).  Samples [0, n) are the records as is;
 * sample n + 8j + 2k + f is record d_sel[j] under rot90^k (np.rot90, axes (1,2))
 * then, if f, np.flip(axis=2).  Outputs: d_x float32 [n+8m][3][15][15] planes
 * [black, white, empty]; d_y int64 move labels (the reference's label map, which
 * rotates the other way, unless GZ_AUG_FIX_LABELS); d_v float32 z.  d_sel values
 * must lie in [0, n) (others give zero planes and label -1). */
#define GZ_AUG_FIX_LABELS 1
int gz_dataset_build(const gz_record* d_records, int32_t n, const int32_t* d_sel, int32_t m, int32_t flags,
                     float* d_x, int64_t* d_y, float* d_v, void* stream);
/* The samples d_ids[0..count) of that dataset (a training batch, e.g. a DataLoader
 * permutation slice) without materialising the rest: outputs [count][...].
 * Ids outside [0, n+8m) give zero planes and label -1. */
int gz_dataset_gather(const gz_record* d_records, int32_t n, const int32_t* d_sel, int32_t m, const int64_t* d_ids,
                      int64_t count, int32_t flags, float* d_x, int64_t* d_y, float* d_v, void* stream);
/* The policy targets of the same samples from PUCT root visit counts (gz_selfplay_puct_run's
 * d_visits, uint16 [n][225], row i belonging to record i): d_pi float32 [count][225],
 * pi[cell] = visits[source(cell)] / sum(visits), where the row moves exactly as the planes
 * of that sample do (rot90^k, then the flip).  A distribution has no analogue of the
 * reference's label map, so GZ_AUG_FIX_LABELS does not apply here: a one-hot row lands on
 * the label that gz_dataset_gather gives with GZ_AUG_FIX_LABELS.  One correctly rounded
 * float32 division per cell (counts are at most 4095, so both operands are exact).
 * d_ids NULL: samples 0..count-1 in order (count = n + 8m is the whole set).  An id
 * outside [0, n+8m), a selection outside [0, n) or a row whose sum is 0 gives a row of
 * NaN (the analogue of label -1: it poisons the loss instead of training on nothing). */
int gz_dataset_pi(const uint16_t* d_visits, int32_t n, const int32_t* d_sel, int32_t m, const int64_t* d_ids,
                  int64_t count, float* d_pi, void* stream);

/* ---- f1 training step: the policy-value net's convolutional part in training mode
 * (training.py:277-311 over neural_network.py:74-91, 132-159: BatchNorm on batch
 * statistics), forward and backward on the device (csrc/gz_sgd.hip):
 *   a0 = relu(BN0(conv0(x))); per block: h = relu(BN1(conv1(a) + b1)), a' = relu(BN2(conv2(h) + b2) + a);
 *   pin = policy_conv(a2) (flattened [boards][2 * 225]), vin = value_conv(a2) ([boards][225])
 * The FC heads (policy_fc, value_fc1/2), the loss and the optimiser stay with the caller
 * (gzero/sgd.py).  x = the model input planes float32 [boards][3][15][15]; activations
 * are fp32 NHWC [boards][225][128] in the workspace.  Weights in torch's layouts:
 * conv0 [128][3][3][3]; residual convs [128][128][3][3] (tower.0.conv1, tower.0.conv2,
 * tower.1.conv1, tower.1.conv2); policy_conv [2][128]; value_conv [1][128].  BN order:
 * bn, tower.0.bn1, tower.0.bn2, tower.1.bn1, tower.1.bn2.  gz_sgd_forward updates the
 * running statistics (momentum, unbiased variance) like torch.nn.BatchNorm2d.train();
 * the workspace (gz_sgd_workspace_bytes) carries the saved activations and statistics
 * from gz_sgd_forward to the gz_sgd_backward of the same batch. */
#define GZ_SGD_MAX_BOARDS 65535
typedef struct gz_sgd_net {
    const float* bn_weight[5];
    const float* bn_bias[5];
    float* bn_running_mean[5]; /* updated in place; NULL: not tracked */
    float* bn_running_var[5];
    const float* conv_weight[4];
    const float* conv_bias[4];
    float momentum, eps;
    const float* conv0_weight;
    const float* conv0_bias;
    const float* policy_weight;
    const float* policy_bias;
    const float* value_weight;
    const float* value_bias;
} gz_sgd_net;
typedef struct gz_sgd_grads { /* outputs (overwritten, not accumulated) */
    float* bn_weight[5];
    float* bn_bias[5];
    float* conv_weight[4];
    float* conv_bias[4];
    float* conv0_weight;
    float* conv0_bias;
    float* policy_weight;
    float* policy_bias;
    float* value_weight;
    float* value_bias;
} gz_sgd_grads;
size_t gz_sgd_workspace_bytes(int32_t boards);
/* d_pin [boards][450], d_vin [boards][225]: the heads' conv outputs of planes d_x */
int gz_sgd_forward(const gz_sgd_net* net, int32_t boards, const float* d_x, float* d_pin, float* d_vin,
                   void* d_workspace, void* stream);
/* from dL/dpin, dL/dvin: every parameter's gradient (d_x and the workspace are the
 * forward's) */
int gz_sgd_backward(const gz_sgd_net* net, int32_t boards, const float* d_x, const float* d_dpin,
                    const float* d_dvin, const gz_sgd_grads* grads, void* d_workspace, void* stream);
/* The FC heads and the loss of the training step (training.py:292-297 over
 * neural_network.py:150-159): logits = policy_fc(pin), val = tanh(value_fc2(relu(
 * value_fc1(vin)))), loss = CrossEntropy(logits, y) + MSE(val, v) (batch means), and
 * its backward: d_dpin [boards][450] and d_dvin [boards][225] for gz_sgd_backward and
 * the six FC gradients (overwritten), all multiplied by `scale` (1, or this rank's
 * share of a data-parallel global batch).  d_y int64 class labels [boards], d_v
 * [boards] targets; d_loss float[3] = {loss, mean cross-entropy, mean squared error}
 * (unscaled).  Weights in torch's layouts: policy_fc [225][450], value_fc1 [64][225],
 * value_fc2 [1][64].  d_ws: gz_sgd_fc_workspace_bytes(boards) bytes. */
typedef struct gz_sgd_fc {
    const float* policy_weight;
    const float* policy_bias;
    const float* value1_weight;
    const float* value1_bias;
    const float* value2_weight;
    const float* value2_bias;
} gz_sgd_fc;
typedef struct gz_sgd_fc_grads {
    float* policy_weight;
    float* policy_bias;
    float* value1_weight;
    float* value1_bias;
    float* value2_weight;
    float* value2_bias;
} gz_sgd_fc_grads;
size_t gz_sgd_fc_workspace_bytes(int32_t boards);
int gz_sgd_fc_loss(const gz_sgd_fc* fc, int32_t boards, const float* d_pin, const float* d_vin, const int64_t* d_y,
                   const float* d_v, float scale, float* d_dpin, float* d_dvin, const gz_sgd_fc_grads* grads,
                   float* d_loss, void* d_ws, void* stream);
/* The same step against probability targets d_pi float32 [boards][225] (the visit
 * distribution of a PUCT search, gz_dataset_pi) in place of class labels: per board
 * ce = sum_i pi_i (logsumexp - logit_i) and dlogits_i = (softmax_i sum(pi) - pi_i) scale /
 * boards, torch's CrossEntropyLoss with probability targets for any non-negative row
 * (normalised or not); d_loss[1] is the mean soft cross-entropy.  The value head and
 * everything else are gz_sgd_fc_loss's, and rows that are exactly one-hot give its outputs
 * bit for bit.  An entry that is not finite or is below 0 makes the loss and every
 * gradient of the step NaN (as a label outside [0, 225) does there). */
int gz_sgd_fc_loss_soft(const gz_sgd_fc* fc, int32_t boards, const float* d_pin, const float* d_vin,
                        const float* d_pi, const float* d_v, float scale, float* d_dpin, float* d_dvin,
                        const gz_sgd_fc_grads* grads, float* d_loss, void* d_ws, void* stream);
/* checkers: a copy of a saved tensor of the last gz_sgd_forward on this workspace:
 * which 0..3 = the inputs of the four residual convs (a0, h1, a1, h2), 4..7 = their
 * outputs y1..y4, 8 = the tower output a2, 9 = y0 = conv0's output (fp32 NHWC) */
int gz_sgd_saved(const void* d_workspace, int32_t boards, int32_t which, float* d_out, void* stream);

/* The optimiser step of training.train_epoch (training.py:303-304): clip_grad_norm_(params,
 * max_norm) then Adam(lr, betas, eps, weight_decay) (torch.optim.Adam, L2 weight decay),
 * over up to GZ_ADAM_MAX_TENSORS tensors in two launches.  max_norm > 0: the gradients are
 * scaled by min(1, max_norm / (||g||_2 + 1e-6)) (the norm over every tensor, summed in
 * float64 in a fixed order: deterministic) -- in place, as clip_grad_norm_ does; max_norm
 * <= 0: no clipping.  step = the step number after this update (1 on the first).  Then per
 * element g' = g + wd p; m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2;
 * p -= (lr / (1-b1^step)) m / (sqrt(v) / sqrt(1-b2^step) + eps).  d_norm (optional): the
 * pre-clip norm (float32, as clip_grad_norm_ returns), written only when max_norm > 0
 * (without clipping no norm is computed and *d_norm keeps its value).  d_workspace:
 * gz_adam_workspace_bytes(). */
#define GZ_ADAM_MAX_TENSORS 48
typedef struct gz_adam_tensor {
    float* param;
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
} gz_adam_tensor;
size_t gz_adam_workspace_bytes(void);
int gz_adam_step(const gz_adam_tensor* tensors, int32_t n_tensors, float lr, float beta1, float beta2, float eps,
                 float weight_decay, int64_t step, float max_norm, float* d_norm, void* d_workspace, void* stream);

#ifdef __cplusplus
}
#endif
