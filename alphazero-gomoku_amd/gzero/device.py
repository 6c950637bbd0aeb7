"""Thin torch-owned-memory wrappers around the libgzero C-ABI.

Every buffer is a torch tensor on the current CUDA(HIP) device; raw pointers
and torch's current stream are handed to the library.  Nothing here runs on the
CPU as a substitute: without a GPU or the library the calls raise.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .boards import RECORD_DTYPE, STATE_DTYPE
from .weights import PRECISIONS


def require_gpu():
    lib = _lib.load()
    if not torch.cuda.is_available():
        raise _lib.GzeroUnavailable("no HIP device visible: the gzero engine has no CPU fallback")
    return lib


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(None)


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def to_dev(arr):
    """numpy array (any dtype) -> uint8 device tensor holding the same bytes."""
    a = np.ascontiguousarray(arr)
    return torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()


def from_dev(t, dtype, count=None):
    a = t.cpu().numpy().view(dtype)
    return a if count is None else a[:count]


def search_params(num_simulations=200, c_puct=1.6, exploration=0.05, beta=0.2, seed=0, max_depth=100,
                  planner_steps=0, gather_leaves=False):
    return _lib.SearchParams(int(num_simulations), int(max_depth), float(c_puct), float(exploration),
                             float(beta), int(seed) & ((1 << 64) - 1), int(planner_steps),
                             _lib.GZ_FLAG_GATHER_LEAVES if gather_leaves else 0)


# ---------------------------------------------------------------- K1 board step
def board_step(states, moves):
    """Batched GomokuBoard.make_move: returns (new states, ok[int32], legal[n,4] uint64)."""
    lib = require_gpu()
    states = np.ascontiguousarray(states, dtype=STATE_DTYPE)
    n = len(states)
    d_states = to_dev(states)
    d_moves = torch.as_tensor(np.asarray(moves, np.int32)).cuda()
    d_ok = torch.empty(n, dtype=torch.int32, device="cuda")
    d_legal = torch.empty(n * 4, dtype=torch.int64, device="cuda")
    _lib.check(lib.gz_board_step(ptr(d_states), ptr(d_moves), n, ptr(d_ok), ptr(d_legal), stream()), "gz_board_step")
    torch.cuda.synchronize()
    return (from_dev(d_states, STATE_DTYPE), d_ok.cpu().numpy(),
            d_legal.cpu().numpy().view(np.uint64).reshape(n, 4))


# ---------------------------------------------------------------- rollout policy
def policy_move(states, keys):
    lib = require_gpu()
    states = np.ascontiguousarray(states, dtype=STATE_DTYPE)
    n = len(states)
    d_states = to_dev(states)
    d_keys = torch.as_tensor(np.asarray(keys, np.uint64).view(np.int64)).cuda()
    d_moves = torch.empty(n, dtype=torch.int32, device="cuda")
    d_draws = torch.empty(n, dtype=torch.int32, device="cuda")
    _lib.check(lib.gz_policy_move(ptr(d_states), ptr(d_keys), n, ptr(d_moves), ptr(d_draws), stream()),
               "gz_policy_move")
    torch.cuda.synchronize()
    return d_moves.cpu().numpy(), d_draws.cpu().numpy()


def rollout(states, ai, keys, max_depth=100):
    lib = require_gpu()
    states = np.ascontiguousarray(states, dtype=STATE_DTYPE)
    n = len(states)
    d_states = to_dev(states)
    d_ai = torch.as_tensor(np.asarray(ai, np.int32)).cuda()
    d_keys = torch.as_tensor(np.asarray(keys, np.uint64).view(np.int64)).cuda()
    d_vals = torch.empty(n, dtype=torch.float64, device="cuda")
    d_fin = torch.empty(n * STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    d_draws = torch.empty(n, dtype=torch.int32, device="cuda")
    _lib.check(lib.gz_rollout(ptr(d_states), ptr(d_ai), ptr(d_keys), n, int(max_depth), ptr(d_vals), ptr(d_fin),
                              ptr(d_draws), stream()), "gz_rollout")
    torch.cuda.synchronize()
    return d_vals.cpu().numpy(), from_dev(d_fin, STATE_DTYPE), d_draws.cpu().numpy()


def pattern_score(states, players):
    lib = require_gpu()
    states = np.ascontiguousarray(states, dtype=STATE_DTYPE)
    n = len(states)
    d_states = to_dev(states)
    d_pl = torch.as_tensor(np.asarray(players, np.int32)).cuda()
    d_s = torch.empty(n, dtype=torch.int64, device="cuda")
    d_bg = torch.empty(n, dtype=torch.float64, device="cuda")
    _lib.check(lib.gz_pattern_score(ptr(d_states), ptr(d_pl), n, ptr(d_s), ptr(d_bg), stream()), "gz_pattern_score")
    torch.cuda.synchronize()
    return d_s.cpu().numpy(), d_bg.cpu().numpy()


# ---------------------------------------------------------------- MCTS get_move
def parse_tree(raw, num_simulations, n_nodes):
    """One exported search tree (LDS layout of gz_selfplay.hip) -> dict of arrays."""
    mn = num_simulations + 1
    b = np.asarray(raw, np.uint8)
    return {
        "value": b[0:8 * mn].view(np.float64)[:n_nodes],
        "bg": b[8 * mn:16 * mn].view(np.float64)[:n_nodes],
        "visits": b[16 * mn:20 * mn].view(np.int32)[:n_nodes],
        "parent": b[20 * mn:22 * mn].view(np.int16)[:n_nodes],
        "bound": b[22 * mn:24 * mn].view(np.int16)[:n_nodes],
        "move": b[24 * mn:25 * mn][:n_nodes],
        "term": b[25 * mn:26 * mn][:n_nodes],
    }


def search(states, game_ids, params, want_trees=False, leaf_cap=0):
    """One AlphaZeroGomokuAI.get_move per state.  Returns (moves, stats, trees, leaves)."""
    lib = require_gpu()
    states = np.ascontiguousarray(states, dtype=STATE_DTYPE)
    n = len(states)
    d_states = to_dev(states)
    d_gids = torch.as_tensor(np.asarray(game_ids, np.int64)).cuda()
    d_moves = torch.empty(n, dtype=torch.int32, device="cuda")
    d_stats = torch.empty(n * ctypes.sizeof(_lib.SearchStats), dtype=torch.uint8, device="cuda")
    tb = lib.gz_tree_bytes(params.num_simulations)
    d_trees = torch.empty(n * tb, dtype=torch.uint8, device="cuda") if want_trees else None
    gather = (params.flags & _lib.GZ_FLAG_GATHER_LEAVES) != 0
    d_leaves = torch.empty(max(1, leaf_cap) * 16, dtype=torch.int32, device="cuda") if gather else None
    # in/out (gzero.h: "*d_leaf_count (the caller zeroes it) is advanced by every leaf produced")
    d_lc = torch.zeros(1, dtype=torch.int32, device="cuda") if gather else None
    _lib.check(lib.gz_search(ptr(d_states), ptr(d_gids), n, ctypes.byref(params), ptr(d_trees), ptr(d_moves),
                             ptr(d_stats), ptr(d_leaves), int(leaf_cap), ptr(d_lc), stream()), "gz_search")
    torch.cuda.synchronize()
    st = np.frombuffer(d_stats.cpu().numpy().tobytes(), dtype=np.dtype(
        [("n_nodes", "<i4"), ("predicts", "<i4"), ("main_draws", "<i4"), ("pad", "<i4"), ("sim_draws", "<i8")]))
    trees = None
    if want_trees:
        raw = d_trees.cpu().numpy().reshape(n, tb)
        trees = [parse_tree(raw[i], params.num_simulations, int(st["n_nodes"][i])) for i in range(n)]
    leaves = None
    if gather:
        cnt = int(d_lc.item())
        leaves = d_leaves.cpu().numpy().view(np.uint32).reshape(-1, 16)[:min(cnt, leaf_cap)]
    return d_moves.cpu().numpy(), st, trees, leaves


# ---------------------------------------------------------------- PV forward
class PVWeights:
    """Packed weight blob resident on the device (+ the fp32 kernel's scratch slab).

    precision: "fp32" (exact f32 MFMA), "f16x3" (3-term fp16 split on the
    fp16 MFMA, f32 accumulation) or "f16" (GZ_PV_F16: one fp16 MFMA per product,
    maps stored as fp16; opt-in, not within 1e-4 of the fp32 forward)."""

    def __init__(self, blob, precision="f16x3"):
        if precision not in PRECISIONS:
            raise ValueError(f"unknown precision {precision!r}")
        lib = require_gpu()
        self.precision = precision
        self.mode = PRECISIONS[precision]
        if isinstance(blob, torch.Tensor):  # (weights.pack_pv_weights_torch: packed on the device)
            blob = blob.detach().to(device="cuda", dtype=torch.float32).contiguous().reshape(-1)
        else:
            blob = torch.from_numpy(np.ascontiguousarray(blob, np.float32).reshape(-1))
        if blob.numel() != lib.gz_pv_weight_floats():
            raise ValueError(f"weight blob has {blob.numel()} floats, kernel expects {lib.gz_pv_weight_floats()}")
        self.tensor = blob.cuda()
        self.workspace = torch.empty(0, dtype=torch.uint8, device="cuda")

    def workspace_for(self, n):
        """gz_pv_workspace_bytes(n) bytes of scratch (the fp32 kernel's slabs, or the f16x3
        tower -> FC-heads records), grown on demand and kept."""
        need = _lib.load().gz_pv_workspace_bytes(int(max(1, n)))
        if self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.uint8, device="cuda")
        return self.workspace


def pv_forward_dev(weights, d_boards, n, d_count=None, d_logits=None, d_value=None, d_probs=None, d_prior=None):
    """Device-resident forward: d_boards int32/uint32 tensor [n,16]; returns output tensors.
    d_prior (float64 [n*225], needs d_probs): MCTSNode._get_prior_probability, dense."""
    lib = require_gpu()
    if d_logits is None:
        d_logits = torch.empty(n * 225, dtype=torch.float32, device="cuda")
    if d_value is None:
        d_value = torch.empty(n, dtype=torch.float32, device="cuda")
    _lib.check(lib.gz_pv_forward(ptr(weights.tensor), ptr(d_boards), int(n), ptr(d_count), ptr(d_logits),
                                 ptr(d_value), ptr(d_probs), ptr(d_prior), ptr(weights.workspace_for(n)),
                                 weights.mode, stream()),
               "gz_pv_forward")
    return d_logits, d_value, d_probs


def pv_forward(weights, leaf_rows, want_prior=False):
    """Host convenience: [n,16] uint32 leaf rows -> (logits [n,225], value [n], probs [n,225])
    (+ prior [n,225] float64, dense over cells, 0 at stones, if want_prior)."""
    rows = np.ascontiguousarray(leaf_rows, np.uint32).reshape(-1, 16)
    n = rows.shape[0]
    d_b = torch.from_numpy(rows.view(np.int32).copy()).cuda()
    d_probs = torch.empty(n * 225, dtype=torch.float32, device="cuda")
    d_prior = torch.empty(n * 225, dtype=torch.float64, device="cuda") if want_prior else None
    lg, v, pr = pv_forward_dev(weights, d_b, n, d_probs=d_probs, d_prior=d_prior)
    torch.cuda.synchronize()
    out = (lg.cpu().numpy().reshape(n, 225), v.cpu().numpy(), pr.cpu().numpy().reshape(n, 225))
    if want_prior:
        out += (d_prior.cpu().numpy().reshape(n, 225),)
    return out


def pv_sym(rows, seed):
    """t uint8 [n] of gz_pv_sym: the board symmetry (0..7, t = 2 k + f) under which the
    leaf-symmetry search evaluates each [16] uint32 row -- a function of (seed, row) alone."""
    lib = require_gpu()
    rows = np.ascontiguousarray(rows, np.uint32).reshape(-1, 16)
    n = rows.shape[0]
    d_b = torch.from_numpy(rows.view(np.int32).copy()).cuda()
    d_t = torch.empty(max(1, n), dtype=torch.uint8, device="cuda")
    _lib.check(lib.gz_pv_sym(ptr(d_b), n, int(seed) & ((1 << 64) - 1), ptr(d_t), stream()), "gz_pv_sym")
    return d_t.cpu().numpy()[:n]


def pv_sym_host(seed, row):
    """gz_pv_sym_host: the same for one row, on the host (no GPU)."""
    row = np.ascontiguousarray(row, np.uint32)
    if row.shape != (16,):
        raise ValueError("row must have 16 words")
    return int(_lib.load().gz_pv_sym_host(int(seed) & ((1 << 64) - 1), row.ctypes.data))


def _sym_workspace(weights, n):
    need = _lib.load().gz_pv_sym_workspace_bytes(int(max(1, n)))
    if weights.workspace.numel() < need:
        weights.workspace = torch.empty(need, dtype=torch.uint8, device="cuda")
    return weights.workspace


def pv_forward_sym_dev(weights, d_boards, n, d_sym=None, seed=0, d_count=None, d_logits=None, d_value=None,
                       d_probs=None, d_prior=None):
    """pv_forward_dev under a board symmetry per row (gz_pv_forward_sym): d_sym uint8 [n]
    on the device, or None for gz_pv_sym(seed, row).  The 225-wide outputs come back in the
    boards' own frame; d_boards is not modified."""
    lib = require_gpu()
    if d_logits is None:
        d_logits = torch.empty(n * 225, dtype=torch.float32, device="cuda")
    if d_value is None:
        d_value = torch.empty(n, dtype=torch.float32, device="cuda")
    _lib.check(lib.gz_pv_forward_sym(ptr(weights.tensor), ptr(d_boards), int(n), ptr(d_count), ptr(d_sym),
                                     int(seed) & ((1 << 64) - 1), ptr(d_logits), ptr(d_value), ptr(d_probs),
                                     ptr(d_prior), ptr(_sym_workspace(weights, n)), weights.mode, stream()),
               "gz_pv_forward_sym")
    return d_logits, d_value, d_probs


def pv_forward_sym(weights, leaf_rows, sym=None, seed=0, want_prior=False):
    """pv_forward under a board symmetry per row: sym uint8 [n] (t = 2 k + f), or None for
    the transform the leaf-symmetry search picks, pv_sym(rows, seed)."""
    rows = np.ascontiguousarray(leaf_rows, np.uint32).reshape(-1, 16)
    n = rows.shape[0]
    d_b = torch.from_numpy(rows.view(np.int32).copy()).cuda()
    d_sym = None
    if sym is not None:
        sym = np.ascontiguousarray(sym, np.uint8).reshape(-1)
        if sym.shape[0] != n:
            raise ValueError("sym wants one transform per row")
        d_sym = torch.from_numpy(sym.copy()).cuda()
    d_probs = torch.empty(n * 225, dtype=torch.float32, device="cuda")
    d_prior = torch.empty(n * 225, dtype=torch.float64, device="cuda") if want_prior else None
    lg, v, pr = pv_forward_sym_dev(weights, d_b, n, d_sym=d_sym, seed=seed, d_probs=d_probs, d_prior=d_prior)
    torch.cuda.synchronize()
    out = (lg.cpu().numpy().reshape(n, 225), v.cpu().numpy(), pr.cpu().numpy().reshape(n, 225))
    if want_prior:
        out += (d_prior.cpu().numpy().reshape(n, 225),)
    return out


def pv_forward_tree(weights, leaf_rows, meta, root_cap=None, d_count=None):
    """Host convenience for gz_pv_forward_tree: [n,16] uint32 leaf rows and their
    int32 meta (-1 root, >= 0 the parent's index for a root child or a child of
    one, -2 other) ->
    (logits [n,225], value [n], probs [n,225], prior [n,225], list sizes).
    d_count (optional, an int): the count-on-device form -- only the first
    min(d_count, n) rows are evaluated; the outputs start as NaN, so a row the
    library did not write stays NaN."""
    lib = require_gpu()
    rows = np.ascontiguousarray(leaf_rows, np.uint32).reshape(-1, 16)
    n = rows.shape[0]
    meta = np.ascontiguousarray(meta, np.int32)
    if root_cap is None:  # a map slot per root and a quarter more: 11.9 patch slots per map slot
        roots = int((meta == -1).sum())
        root_cap = roots + (roots + 3) // 4
    d_b = torch.from_numpy(rows.view(np.int32).copy()).cuda()
    d_m = torch.from_numpy(meta.copy()).cuda()
    new = torch.empty
    if d_count is not None:
        d_count = torch.tensor([int(d_count)], dtype=torch.int32, device="cuda")
        new = lambda *a, **k: torch.full(*a, float("nan"), **k)  # noqa: E731
    d_lg = new((n * 225,), dtype=torch.float32, device="cuda")
    d_v = new((n,), dtype=torch.float32, device="cuda")
    d_p = new((n * 225,), dtype=torch.float32, device="cuda")
    d_pr = new((n * 225,), dtype=torch.float64, device="cuda")
    ws = torch.empty(lib.gz_pv_tree_workspace_bytes(n, root_cap), dtype=torch.uint8, device="cuda")
    _lib.check(lib.gz_pv_forward_tree(ptr(weights.tensor), ptr(d_b), ptr(d_m), n, ptr(d_count), int(root_cap),
                                      ptr(d_lg), ptr(d_v), ptr(d_p), ptr(d_pr), ptr(ws), stream()),
               "gz_pv_forward_tree")
    st = torch.empty(6, dtype=torch.int32, device="cuda")
    _lib.check(lib.gz_pv_tree_stats(ptr(ws), n, ptr(st), stream()), "gz_pv_tree_stats")
    torch.cuda.synchronize()
    return (d_lg.cpu().numpy().reshape(n, 225), d_v.cpu().numpy(), d_p.cpu().numpy().reshape(n, 225),
            d_pr.cpu().numpy().reshape(n, 225), [int(x) for x in st.cpu()])


class GNWeights:
    """BG planner nets (GraphNet + OpponentDQN) blob resident on the device."""

    def __init__(self, blob):
        lib = require_gpu()
        blob = np.ascontiguousarray(blob, np.float32)
        if blob.size != lib.gz_gn_weight_floats():
            raise ValueError(f"planner blob has {blob.size} floats, kernel expects {lib.gz_gn_weight_floats()}")
        self.tensor = torch.from_numpy(blob).cuda()
        self._ws = None

    def workspace_for(self, n):
        """Device workspace of gz_gn_forward for n boards (grown on demand, kept)."""
        need = int(require_gpu().gz_gn_workspace_bytes(max(1, int(n))))
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device="cuda")
        return self._ws


def gn_forward_dev(weights, d_boards, n, d_count=None, d_p=None, d_q=None, d_logits=None):
    lib = require_gpu()
    if d_p is None:
        d_p = torch.empty(n * 225, dtype=torch.float32, device="cuda")
    if d_q is None:
        d_q = torch.empty(n * 225, dtype=torch.float32, device="cuda")
    _lib.check(lib.gz_gn_forward(ptr(weights.tensor), ptr(d_boards), int(n), ptr(d_count), ptr(d_p), ptr(d_q),
                                 ptr(d_logits), ptr(weights.workspace_for(n)), stream()), "gz_gn_forward")
    return d_p, d_q, d_logits


def gn_forward(weights, leaf_rows):
    """Host convenience: [n,16] uint32 rows -> (p [n,225], q [n,225], logits [n,225])."""
    rows = np.ascontiguousarray(leaf_rows, np.uint32).reshape(-1, 16)
    n = rows.shape[0]
    d_b = torch.from_numpy(rows.view(np.int32).copy()).cuda()
    d_lg = torch.empty(n * 225, dtype=torch.float32, device="cuda")
    p, q, lg = gn_forward_dev(weights, d_b, n, d_logits=d_lg)
    torch.cuda.synchronize()
    return p.cpu().numpy().reshape(n, 225), q.cpu().numpy().reshape(n, 225), lg.cpu().numpy().reshape(n, 225)


def plan_search(states, game_ids, params, pparams, gn_weights, want_trees=False, leaf_cap=0):
    """AlphaZeroGomokuAI.get_move with BG-planner rollout plies (gz_plan_search).
    Returns (moves, stats, trees, leaves) like search()."""
    lib = require_gpu()
    states = np.ascontiguousarray(states, dtype=STATE_DTYPE)
    n = len(states)
    d_states = to_dev(states)
    d_gids = torch.as_tensor(np.asarray(game_ids, np.int64)).cuda()
    d_moves = torch.empty(n, dtype=torch.int32, device="cuda")
    d_stats = torch.empty(n * ctypes.sizeof(_lib.SearchStats), dtype=torch.uint8, device="cuda")
    S = params.num_simulations
    tb = lib.gz_tree_bytes(S)
    d_trees = torch.empty(n * tb, dtype=torch.uint8, device="cuda") if want_trees else None
    gather = (params.flags & _lib.GZ_FLAG_GATHER_LEAVES) != 0
    d_leaves = torch.empty(max(1, leaf_cap) * 16, dtype=torch.int32, device="cuda") if gather else None
    # in/out (gzero.h: "*d_leaf_count (the caller zeroes it) is advanced by every leaf produced")
    d_lc = torch.zeros(1, dtype=torch.int32, device="cuda") if gather else None
    ws = torch.empty(lib.gz_plan_workspace_bytes(n, S), dtype=torch.uint8, device="cuda")
    _lib.check(lib.gz_plan_search(ptr(d_states), ptr(d_gids), n, ctypes.byref(params), ctypes.byref(pparams),
                                  ptr(gn_weights.tensor), ptr(ws), ptr(d_trees), ptr(d_moves), ptr(d_stats),
                                  ptr(d_leaves), int(leaf_cap), ptr(d_lc), stream()), "gz_plan_search")
    torch.cuda.synchronize()
    st = np.frombuffer(d_stats.cpu().numpy().tobytes(), dtype=np.dtype(
        [("n_nodes", "<i4"), ("predicts", "<i4"), ("main_draws", "<i4"), ("pad", "<i4"), ("sim_draws", "<i8")]))
    trees = None
    if want_trees:
        raw = d_trees.cpu().numpy().reshape(n, tb)
        trees = [parse_tree(raw[i], S, int(st["n_nodes"][i])) for i in range(n)]
    leaves = None
    if gather:
        cnt = int(d_lc.item())
        leaves = d_leaves.cpu().numpy().view(np.uint32).reshape(-1, 16)[:min(cnt, leaf_cap)]
    return d_moves.cpu().numpy(), st, trees, leaves


# ---------------------------------------------------------------- PUCT search
def puct_params(num_simulations=200, c_puct=1.6, temp_plies=0, seed=0, precision="f16x3", dirichlet_alpha=None,
                noise_eps=0.25, leaves_per_round=1, fast_simulations=None, full_prob=0.25, leaf_symmetry=False,
                forced_playouts=None, gumbel_considered=None, c_visit=50.0, c_scale=0.5, gumbel_scale=1.0):
    """gz_puct_params; precision ("fp32" / "f16x3" / "f16") is the forward gz_puct_search runs.
    dirichlet_alpha: Dirichlet noise at the search root, prior' = (1 - noise_eps) prior +
    noise_eps Dir(dirichlet_alpha) over the empty cells, once per root (include/gzero.h);
    the result is then a gz_puct_noise_params with GZ_PUCT_ROOT_NOISE set.  None (the
    default): no noise, the plain 32-byte struct.
    leaves_per_round K > 1: leaf batching with virtual loss, K leaves per game per round
    (a gz_puct_batch_params with GZ_PUCT_LEAF_BATCH set); 1 (the default) is the
    unbatched search with the flag clear.
    fast_simulations F: playout cap randomization (a gz_puct_cap_params with
    GZ_PUCT_PLAYOUT_CAP set): every ply is a full search of num_simulations with
    probability full_prob, else a fast one of F simulations without root noise
    (include/gzero.h).  None (the default): no cap, full_prob is not read.  Not with
    leaves_per_round > 1.
    leaf_symmetry: every leaf is evaluated under one of the 8 board symmetries, picked by
    (seed, position), and its prior mapped back (GZ_PUCT_LEAF_SYM; the struct is the one
    the other options give).  False (the default): the flag is clear.
    forced_playouts k: forced playouts at full-budget roots and pruning of the visit rows
    that leave the search (a gz_puct_forced_params with GZ_PUCT_FORCED_PLAYOUTS set;
    include/gzero.h), k finite and in [0, 16] (KataGo: 2; 0 forces and prunes nothing).
    None (the default): the flag is clear.  Not with leaves_per_round > 1.
    gumbel_considered m: the Gumbel root with sequential halving (a gz_puct_gumbel_params with
    GZ_PUCT_GUMBEL set; include/gzero.h): m in [1, 32] root moves sampled without replacement,
    the budget spent by halving, the move and the policy target from logits + sigma(q) with
    sigma(q) = (c_visit + max visits) c_scale q (q in [-1, 1]: c_scale 0.5 is the paper's 1.0),
    gumbel_scale 0 for the deterministic variant.  None (the default): the flag is clear and
    c_visit, c_scale, gumbel_scale are not read.  Only with leaf_symmetry among the options."""
    if gumbel_considered is not None:
        if dirichlet_alpha is not None or int(leaves_per_round) != 1 or fast_simulations is not None \
                or forced_playouts is not None:
            raise ValueError("gumbel_considered is not supported with dirichlet_alpha, leaves_per_round > 1, "
                             "fast_simulations or forced_playouts")
        return _with_gumbel(puct_params(num_simulations, c_puct, temp_plies, seed, precision,
                                        leaf_symmetry=leaf_symmetry), gumbel_considered, c_visit, c_scale, gumbel_scale)
    if forced_playouts is not None:
        return _with_forced(puct_params(num_simulations, c_puct, temp_plies, seed, precision, dirichlet_alpha,
                                        noise_eps, leaves_per_round, fast_simulations, full_prob, leaf_symmetry),
                            forced_playouts)
    if leaf_symmetry:
        p = puct_params(num_simulations, c_puct, temp_plies, seed, precision, dirichlet_alpha, noise_eps,
                        leaves_per_round, fast_simulations, full_prob)
        p.flags |= _lib.GZ_PUCT_LEAF_SYM
        return p
    if fast_simulations is not None:
        return _with_cap(puct_params(num_simulations, c_puct, temp_plies, seed, precision, dirichlet_alpha, noise_eps,
                                     leaves_per_round), fast_simulations, full_prob)
    if precision not in PRECISIONS:
        raise ValueError(f"unknown precision {precision!r}")
    mode = PRECISIONS[precision]
    base = (int(num_simulations), int(temp_plies), float(c_puct), int(seed) & ((1 << 64) - 1), mode)
    K = int(leaves_per_round)
    if not 1 <= K <= _lib.GZ_PUCT_MAX_LEAVES:
        raise ValueError(f"leaves_per_round must be in [1, {_lib.GZ_PUCT_MAX_LEAVES}], not {leaves_per_round!r}")
    batch = _lib.GZ_PUCT_LEAF_BATCH if K > 1 else 0
    if dirichlet_alpha is None:
        return _lib.PuctBatchParams(*base, batch, 0.0, 0.0, K, 0) if batch else _lib.PuctParams(*base, 0)
    alpha, eps = float(dirichlet_alpha), float(noise_eps)
    if not 1e-3 <= alpha <= 1e3:
        raise ValueError(f"dirichlet_alpha must be in [1e-3, 1e3], not {dirichlet_alpha!r}")
    if not 0.0 <= eps <= 1.0:
        raise ValueError(f"noise_eps must be in [0, 1], not {noise_eps!r}")
    if batch:
        return _lib.PuctBatchParams(*base, _lib.GZ_PUCT_ROOT_NOISE | batch, alpha, eps, K, 0)
    return _lib.PuctNoiseParams(*base, _lib.GZ_PUCT_ROOT_NOISE, alpha, eps)


def _with_cap(params, fast_simulations, full_prob):
    """The gz_puct_cap_params of uncapped, unbatched params."""
    F, prob = int(fast_simulations), float(full_prob)
    if params.flags & _lib.GZ_PUCT_LEAF_BATCH:
        raise ValueError("fast_simulations (the playout cap) is not supported with leaves_per_round > 1")
    if not 1 <= F <= params.num_simulations:
        raise ValueError(f"fast_simulations must be in [1, num_simulations], not {fast_simulations!r}")
    if not 0.0 <= prob <= 1.0:  # (a NaN fails both)
        raise ValueError(f"full_prob must be in [0, 1], not {full_prob!r}")
    noise = params.flags & _lib.GZ_PUCT_ROOT_NOISE
    sym = params.flags & _lib.GZ_PUCT_LEAF_SYM
    alpha, eps = (params.noise_alpha, params.noise_eps) if noise else (0.0, 0.0)
    return _lib.PuctCapParams(params.num_simulations, params.temp_plies, params.c_puct, params.seed, params.precision,
                              noise | sym | _lib.GZ_PUCT_PLAYOUT_CAP, alpha, eps, 1, 0, F, 0, prob)


def _with_forced(params, forced_playouts):
    """The gz_puct_forced_params of unbatched params; the inner fields of the options that
    are off are zero and not read."""
    k = float(forced_playouts)
    if params.flags & _lib.GZ_PUCT_LEAF_BATCH:
        raise ValueError("forced_playouts is not supported with leaves_per_round > 1")
    if not 0.0 <= k <= 16.0:  # (a NaN fails both)
        raise ValueError(f"forced_playouts must be in [0, 16], not {forced_playouts!r}")
    noise = params.flags & _lib.GZ_PUCT_ROOT_NOISE
    cap = params.flags & _lib.GZ_PUCT_PLAYOUT_CAP
    alpha, eps = (params.noise_alpha, params.noise_eps) if noise else (0.0, 0.0)
    F, prob = (params.fast_simulations, params.full_prob) if cap else (0, 0.0)
    return _lib.PuctForcedParams(params.num_simulations, params.temp_plies, params.c_puct, params.seed,
                                 params.precision, params.flags | _lib.GZ_PUCT_FORCED_PLAYOUTS, alpha, eps, 1, 0, F, 0,
                                 prob, k)


def _with_gumbel(params, gumbel_considered, c_visit=50.0, c_scale=0.5, gumbel_scale=1.0):
    """The gz_puct_gumbel_params of plain params (leaf_symmetry allowed); the inner fields
    of the other options are zero and not read."""
    m, cv, cs, gsc = int(gumbel_considered), float(c_visit), float(c_scale), float(gumbel_scale)
    if params.flags & ~_lib.GZ_PUCT_LEAF_SYM:
        raise ValueError("gumbel_considered is not supported with dirichlet_alpha, leaves_per_round > 1, "
                         "fast_simulations or forced_playouts")
    if not 1 <= m <= _lib.GZ_PUCT_GUMBEL_MAX_CONSIDERED:
        raise ValueError(f"gumbel_considered must be in [1, {_lib.GZ_PUCT_GUMBEL_MAX_CONSIDERED}], "
                         f"not {gumbel_considered!r}")
    if not 0.0 <= cv <= 1e4:  # (a NaN fails both)
        raise ValueError(f"c_visit must be in [0, 1e4], not {c_visit!r}")
    if not 0.0 <= cs <= 1e3:
        raise ValueError(f"c_scale must be in [0, 1e3], not {c_scale!r}")
    if not 0.0 <= gsc <= 8.0:
        raise ValueError(f"gumbel_scale must be in [0, 8], not {gumbel_scale!r}")
    return _lib.PuctGumbelParams(params.num_simulations, params.temp_plies, params.c_puct, params.seed,
                                 params.precision, params.flags | _lib.GZ_PUCT_GUMBEL, 0.0, 0.0, 1, 0, 0, 0, 0.0, 0.0,
                                 m, 0, cv, cs, gsc)


def puct_gumbel_sequence_host(m, num_simulations):
    """seq(m, S) int16 [S] of gz_puct_gumbel_sequence_host (no GPU): the visit count the
    considered child selected at each simulation has."""
    lib = _lib.load()
    out = np.zeros(max(1, int(num_simulations)), np.int16)
    _lib.check(lib.gz_puct_gumbel_sequence_host(int(m), int(num_simulations), out.ctypes.data),
               "gz_puct_gumbel_sequence_host")
    return out


def puct_gumbel_root_host(seed, game_id, ply, prior, empty, max_considered, gumbel_scale=1.0):
    """gs float64 [225] of gz_puct_gumbel_root_host (no GPU): g + logit at the considered
    cells, -inf elsewhere; prior float64 [225], empty = 225 truth values."""
    lib = _lib.load()
    pr = np.ascontiguousarray(prior, np.float64)
    e = np.ascontiguousarray(np.asarray(empty).astype(bool), np.uint8)
    if pr.shape != (225,) or e.shape != (225,):
        raise ValueError("prior and empty must have 225 entries")
    out = np.zeros(225, np.float64)
    _lib.check(lib.gz_puct_gumbel_root_host(int(seed) & ((1 << 64) - 1), int(game_id), int(ply), pr.ctypes.data,
                                            e.ctypes.data, int(max_considered), float(gumbel_scale), out.ctypes.data),
               "gz_puct_gumbel_root_host")
    return out


def puct_gumbel_policy_host(prior, W, visits, v0, c_visit=50.0, c_scale=0.5):
    """(pi float64 [225], row int32 [225]) of gz_puct_gumbel_policy_host (no GPU): prior and
    W float64 [225] (prior 0.0 at stones), visits int32 [225] with 0 where the root has no
    child, v0 the root's value."""
    lib = _lib.load()
    pr = np.ascontiguousarray(prior, np.float64)
    w = np.ascontiguousarray(W, np.float64)
    v = np.ascontiguousarray(visits, np.int32)
    if pr.shape != (225,) or w.shape != (225,) or v.shape != (225,):
        raise ValueError("prior, W and visits must have 225 entries")
    pi, row = np.zeros(225, np.float64), np.zeros(225, np.int32)
    _lib.check(lib.gz_puct_gumbel_policy_host(pr.ctypes.data, w.ctypes.data, v.ctypes.data, float(v0), float(c_visit),
                                              float(c_scale), pi.ctypes.data, row.ctypes.data),
               "gz_puct_gumbel_policy_host")
    return pi, row


def forced_prune_host(c_puct, forced_k, root_visits, prior, W, visits):
    """The pruned visit row int32 [225] of gz_puct_forced_prune_host (no GPU): prior and W
    float64 [225], visits int32 [225] with 0 where the root has no child."""
    lib = _lib.load()
    pr = np.ascontiguousarray(prior, np.float64)
    w = np.ascontiguousarray(W, np.float64)
    v = np.ascontiguousarray(visits, np.int32)
    if pr.shape != (225,) or w.shape != (225,) or v.shape != (225,):
        raise ValueError("prior, W and visits must have 225 entries")
    out = np.empty(225, np.int32)
    _lib.check(lib.gz_puct_forced_prune_host(float(c_puct), float(forced_k), int(root_visits), pr.ctypes.data,
                                             w.ctypes.data, v.ctypes.data, out.ctypes.data),
               "gz_puct_forced_prune_host")
    return out


def cap_full(records_dev, seed, full_prob):
    """Which records are full plies of a capped run with this seed and full_prob
    (gz_puct_cap_full): records_dev a device uint8 tensor of gz_record (80 bytes each),
    as SelfPlayEngine.records_device gives it; returns a device bool tensor [n]."""
    lib = require_gpu()
    prob = float(full_prob)
    if not 0.0 <= prob <= 1.0:
        raise ValueError(f"full_prob must be in [0, 1], not {full_prob!r}")
    n = records_dev.numel() // 80
    d_full = torch.empty(n, dtype=torch.uint8, device="cuda")
    _lib.check(lib.gz_puct_cap_full(ptr(records_dev), n, int(seed) & ((1 << 64) - 1), prob, ptr(d_full), stream()),
               "gz_puct_cap_full")
    return d_full != 0


def puct_leaves(params):
    """K of a batched params struct (GZ_PUCT_LEAF_BATCH), 0 for the unbatched search."""
    return int(params.leaves_per_round) if params.flags & _lib.GZ_PUCT_LEAF_BATCH else 0


def with_leaves(params, leaves_per_round):
    """params with another leaves_per_round (None: params as they are; 1 on unbatched
    params: as they are too)."""
    if leaves_per_round is None:
        return params
    K = int(leaves_per_round)
    if not 1 <= K <= _lib.GZ_PUCT_MAX_LEAVES:
        raise ValueError(f"leaves_per_round must be in [1, {_lib.GZ_PUCT_MAX_LEAVES}], not {leaves_per_round!r}")
    if K == 1 and not params.flags & _lib.GZ_PUCT_LEAF_BATCH:
        return params
    if params.flags & _lib.GZ_PUCT_PLAYOUT_CAP:
        raise ValueError("leaves_per_round > 1 is not supported with fast_simulations (the playout cap)")
    if params.flags & _lib.GZ_PUCT_FORCED_PLAYOUTS:
        raise ValueError("leaves_per_round > 1 is not supported with forced_playouts")
    if params.flags & _lib.GZ_PUCT_GUMBEL:
        raise ValueError("leaves_per_round > 1 is not supported with gumbel_considered")
    noise = params.flags & _lib.GZ_PUCT_ROOT_NOISE
    sym = params.flags & _lib.GZ_PUCT_LEAF_SYM
    flags = noise | sym | (_lib.GZ_PUCT_LEAF_BATCH if K > 1 else 0)
    base = (params.num_simulations, params.temp_plies, params.c_puct, params.seed, params.precision)
    alpha, eps = (params.noise_alpha, params.noise_eps) if noise else (0.0, 0.0)
    if K > 1:
        return _lib.PuctBatchParams(*base, flags, alpha, eps, K, 0)
    return _lib.PuctNoiseParams(*base, flags, alpha, eps) if noise else _lib.PuctParams(*base, sym)


def _puct_workspace_bytes(lib, n, params):
    # (an S out of range is the library's error to report: size the workspace for a legal one)
    S = max(0, min(params.num_simulations, _lib.GZ_MAX_SIMULATIONS))
    K = puct_leaves(params)
    size = lib.gz_puct_batch_workspace_bytes(n, S, K) if K else lib.gz_puct_workspace_bytes(n, S)
    return puct_extra_bytes(lib, size, n * max(1, K), n, params)


def puct_extra_bytes(lib, size, rows, n, params):
    """The workspace of `size` flag-clear bytes with what the params' options put behind it:
    gz_puct_sym_bytes(rows) with GZ_PUCT_LEAF_SYM, then, rounded up to 256,
    gz_puct_gumbel_bytes(n, S, max_considered) with GZ_PUCT_GUMBEL."""
    size += puct_sym_bytes(lib, rows, params)
    if params.flags & _lib.GZ_PUCT_GUMBEL:
        S = max(1, min(params.num_simulations, _lib.GZ_MAX_SIMULATIONS))
        size = ((size + 255) & ~255) + lib.gz_puct_gumbel_bytes(int(n), S, int(params.max_considered))
    return size


def puct_sym_bytes(lib, rows, params):
    """What GZ_PUCT_LEAF_SYM adds behind a flag-clear workspace (0 with the flag clear)."""
    return lib.gz_puct_sym_bytes(int(rows)) if params.flags & _lib.GZ_PUCT_LEAF_SYM else 0


def puct_root_noise(states, game_ids, seed, alpha):
    """eta float64 [n,225] of gz_puct_root_noise: the Dirichlet(alpha) sample the search
    mixes into the root of each state (ply = n_moves), 0 at stones."""
    lib = require_gpu()
    states = np.ascontiguousarray(states, dtype=STATE_DTYPE)
    n = len(states)
    d_states = to_dev(states)
    d_gids = torch.as_tensor(np.asarray(game_ids, np.int64)).cuda()
    d_eta = torch.empty(n * 225, dtype=torch.float64, device="cuda")
    _lib.check(lib.gz_puct_root_noise(ptr(d_states), ptr(d_gids), n, int(seed) & ((1 << 64) - 1), float(alpha),
                                      ptr(d_eta), stream()), "gz_puct_root_noise")
    return d_eta.cpu().numpy().reshape(n, 225)


def puct_root_noise_host(seed, game_id, ply, empty, alpha):
    """eta float64 [225] of gz_puct_root_noise_host (no GPU): empty = 225 truth values."""
    lib = _lib.load()
    e = np.ascontiguousarray(np.asarray(empty).astype(bool), np.uint8)
    if e.shape != (225,):
        raise ValueError("empty must have 225 entries")
    out = np.zeros(225, np.float64)
    _lib.check(lib.gz_puct_root_noise_host(int(seed) & ((1 << 64) - 1), int(game_id), int(ply), e.ctypes.data,
                                           float(alpha), out.ctypes.data), "gz_puct_root_noise_host")
    return out


def parse_puct_tree(raw, num_simulations):
    """One exported PUCT tree (gz_puct_trees, layout in csrc/gz_puct.hip) -> dict:
    n_nodes, n_evals, main_draws, move and, per node in creation order, W, prior
    [k,225], visits, value, board [k,16], parent, move_of (255 = root), term."""
    M = num_simulations + 1
    b = np.asarray(raw, np.uint8)
    hdr = b[:16].view(np.int32)
    k = int(hdr[0])
    o = 16
    out = {"n_nodes": k, "n_evals": int(hdr[1]), "main_draws": int(hdr[2]), "move": int(hdr[3])}
    for name, dt, width in (("W", np.float64, 1), ("prior", np.float64, 225), ("visits", np.int32, 1),
                            ("value", np.float32, 1), ("board", np.uint32, 16), ("parent", np.int16, 1),
                            ("move_of", np.uint8, 1), ("term", np.uint8, 1)):
        nb = np.dtype(dt).itemsize * width * M
        a = b[o:o + nb].view(dt)
        out[name] = (a.reshape(M, width)[:k] if width > 1 else a[:k]).copy()
        o += nb
    return out


def _puct_trees(lib, ws, n, S):
    tb = lib.gz_puct_tree_bytes(S)
    d_out = torch.empty(n * tb, dtype=torch.uint8, device="cuda")
    _lib.check(lib.gz_puct_trees(ptr(ws), n, S, ptr(d_out), stream()), "gz_puct_trees")
    raw = d_out.cpu().numpy().reshape(n, tb)
    return [parse_puct_tree(raw[i], S) for i in range(n)]


def puct_search(states, game_ids, params, pv_weights, want_trees=False, leaves_per_round=None):
    """One network-guided PUCT search per state (gz_puct_search) with the forward of
    params.precision.  Returns (moves int32 [n] (-1: the board is over), visits int32
    [n,225] root-child visits, root_q float64 [n], trees or None).  leaves_per_round:
    None = as params say (puct_params(leaves_per_round=...)), else that many leaves per
    game per round."""
    lib = require_gpu()
    params = with_leaves(params, leaves_per_round)
    states = np.ascontiguousarray(states, dtype=STATE_DTYPE)
    n = len(states)
    S = params.num_simulations
    d_states = to_dev(states)
    d_gids = torch.as_tensor(np.asarray(game_ids, np.int64)).cuda()
    d_moves = torch.empty(n, dtype=torch.int32, device="cuda")
    d_visits = torch.empty(n * 225, dtype=torch.int32, device="cuda")
    d_q = torch.empty(n, dtype=torch.float64, device="cuda")
    ws = torch.empty(_puct_workspace_bytes(lib, n, params), dtype=torch.uint8, device="cuda")
    _lib.check(lib.gz_puct_search(ptr(d_states), ptr(d_gids), n, ctypes.byref(params), ptr(pv_weights.tensor),
                                  ptr(ws), ptr(d_moves), ptr(d_visits), ptr(d_q), stream()), "gz_puct_search")
    torch.cuda.synchronize()
    trees = _puct_trees(lib, ws, n, S) if want_trees else None
    return d_moves.cpu().numpy(), d_visits.cpu().numpy().reshape(n, 225), d_q.cpu().numpy(), trees


class PuctStepper:
    """The step API of the PUCT search, for a caller that evaluates the leaves itself:

        st = PuctStepper(states, game_ids, params)       # gz_puct_begin
        rows, active = st.leaves()                       # root boards
        st.backup(prior, value)                          # their evaluation
        for _ in range(S):
            st.select(); rows, active = st.leaves(); st.backup(prior, value)
        moves, visits, root_q = st.finish()

    prior float64 [n,225] and value float32 [n] in gz_pv_forward's layouts (device
    tensors or arrays); rows of inactive games are ignored.

    With a playout cap (puct_params(fast_simulations=...)) a search has no fixed number of
    rounds either: ``remaining()`` (and ``reroot()``'s result) count against each game's own
    budget, and a game at or past it has an inactive row.

    With forced playouts (puct_params(forced_playouts=k)) nothing changes for the caller:
    ``select()`` forces at full-budget roots, ``finish()`` returns the pruned visit rows and
    picks the moves from the raw counts, ``trees()`` shows the raw counts.

    With the Gumbel root (puct_params(gumbel_considered=m)) the calls are the same: ``backup()``
    of the roots prepares the considered moves, ``select()`` follows the halving schedule at the
    root, ``finish()`` returns the improved-policy rows (scaled to 32767) and the moves;
    ``reroot()`` is an error.

    With leaves_per_round K > 1 (here or in params) every buffer has n K rows, game g at
    rows g K .. g K + K - 1, and a search is no fixed number of rounds: after the root's
    backup, ``while st.remaining().any(): st.select(); ...; st.backup(prior, value)``."""

    def __init__(self, states, game_ids, params, leaves_per_round=None):
        self.lib = require_gpu()
        states = np.ascontiguousarray(states, dtype=STATE_DTYPE)
        params = with_leaves(params, leaves_per_round)
        self.n = len(states)
        self.S = params.num_simulations
        self.K = puct_leaves(params)
        self.rows = self.n * max(1, self.K)
        self.params = params
        d_states = to_dev(states)
        d_gids = torch.as_tensor(np.asarray(game_ids, np.int64)).cuda()
        self.d_leaves = torch.empty(self.rows * 16, dtype=torch.int32, device="cuda")
        self.d_active = torch.empty(self.rows, dtype=torch.int32, device="cuda")
        self.ws = torch.empty(_puct_workspace_bytes(self.lib, self.n, params), dtype=torch.uint8, device="cuda")
        _lib.check(self.lib.gz_puct_begin(ptr(d_states), ptr(d_gids), self.n, ctypes.byref(params), ptr(self.ws),
                                          ptr(self.d_leaves), ptr(self.d_active), stream()), "gz_puct_begin")

    def leaves(self):
        """(rows uint32 [n K,16], active bool [n K]) of the current round (synchronising)."""
        rows = self.d_leaves.cpu().numpy().view(np.uint32).reshape(self.rows, 16)
        return rows, self.d_active.cpu().numpy() != 0

    def remaining(self):
        """Simulations left to each game's budget, int32 [n] (0: the game is over or its
        search is finished); gz_puct_remaining, synchronising."""
        d_rem = torch.empty(self.n, dtype=torch.int32, device="cuda")
        _lib.check(self.lib.gz_puct_remaining(ptr(self.ws), self.n, self.S, ptr(d_rem), stream()),
                   "gz_puct_remaining")
        return d_rem.cpu().numpy()

    def select(self):
        _lib.check(self.lib.gz_puct_select(ptr(self.ws), self.n, self.S, ptr(self.d_leaves), ptr(self.d_active),
                                           stream()), "gz_puct_select")

    def backup(self, prior, value):
        if not isinstance(prior, torch.Tensor):
            prior = torch.from_numpy(np.ascontiguousarray(prior, np.float64).reshape(-1)).cuda()
        if not isinstance(value, torch.Tensor):
            value = torch.from_numpy(np.ascontiguousarray(value, np.float32).reshape(-1)).cuda()
        if prior.dtype != torch.float64 or prior.numel() != self.rows * 225 or value.dtype != torch.float32 \
                or value.numel() != self.rows:
            raise ValueError("backup() wants prior float64 [n,225] and value float32 [n] (n K rows when batched)")
        _lib.check(self.lib.gz_puct_backup(ptr(self.ws), self.n, self.S, ptr(prior), ptr(value), stream()),
                   "gz_puct_backup")

    def evaluate(self, weights):
        """The current round's leaves through the network, for backup(): (prior, value)
        device tensors.  With leaf_symmetry in params the step API leaves the transform to
        its caller, so this is pv_forward_sym_dev with the params' seed; without it,
        pv_forward_dev.  weights.mode is the precision (params.precision is not read)."""
        d_probs = torch.empty(self.rows * 225, dtype=torch.float32, device="cuda")
        d_prior = torch.empty(self.rows * 225, dtype=torch.float64, device="cuda")
        if self.params.flags & _lib.GZ_PUCT_LEAF_SYM:
            _, v, _ = pv_forward_sym_dev(weights, self.d_leaves, self.rows, seed=self.params.seed, d_probs=d_probs,
                                         d_prior=d_prior)
        else:
            _, v, _ = pv_forward_dev(weights, self.d_leaves, self.rows, d_probs=d_probs, d_prior=d_prior)
        return d_prior, v

    def finish(self):
        d_moves = torch.empty(self.n, dtype=torch.int32, device="cuda")
        d_visits = torch.empty(self.n * 225, dtype=torch.int32, device="cuda")
        d_q = torch.empty(self.n, dtype=torch.float64, device="cuda")
        _lib.check(self.lib.gz_puct_finish(ptr(self.ws), self.n, self.S, ptr(d_moves), ptr(d_visits), ptr(d_q),
                                           stream()), "gz_puct_finish")
        torch.cuda.synchronize()
        return d_moves.cpu().numpy(), d_visits.cpu().numpy().reshape(self.n, 225), d_q.cpu().numpy()

    def reroot(self, moves):
        """Play moves[g] (row-major cell, -1: leave the game as it is) at every root and
        keep the subtree under it as the next search's tree (gz_puct_reroot).  Returns
        the simulations left to each game's budget, int32 [n] (0: the game is over).
        The next search is then: while any game has simulations left, select(),
        leaves(), backup() -- a game at its budget has an inactive row.  A move
        without a node gives a fresh root whose board is in leaves() right away: back
        it up before the first select()."""
        d_moves = torch.as_tensor(np.asarray(moves, np.int32).reshape(-1)).cuda()
        if d_moves.numel() != self.n:
            raise ValueError("reroot() wants one move per game")
        d_rem = torch.empty(self.n, dtype=torch.int32, device="cuda")
        _lib.check(self.lib.gz_puct_reroot(ptr(self.ws), self.n, self.S, ptr(d_moves), ptr(self.d_leaves),
                                           ptr(self.d_active), ptr(d_rem), stream()), "gz_puct_reroot")
        return d_rem.cpu().numpy()

    def trees(self):
        torch.cuda.synchronize()
        return _puct_trees(self.lib, self.ws, self.n, self.S)


def planner_move(states, ais, keys, pparams, gn_weights):
    """BGPlannerAI.get_move per state (gz_planner_move): returns (moves, draws)."""
    lib = require_gpu()
    states = np.ascontiguousarray(states, dtype=STATE_DTYPE)
    n = len(states)
    d_states = to_dev(states)
    d_ai = torch.as_tensor(np.asarray(ais, np.int32)).cuda()
    d_keys = torch.as_tensor(np.asarray(keys, np.uint64).view(np.int64)).cuda()
    d_moves = torch.empty(n, dtype=torch.int32, device="cuda")
    d_draws = torch.empty(n, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.gz_planner_move_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    _lib.check(lib.gz_planner_move(ptr(d_states), ptr(d_ai), ptr(d_keys), n, ctypes.byref(pparams),
                                   ptr(gn_weights.tensor), ptr(ws), ptr(d_moves), ptr(d_draws), stream()),
               "gz_planner_move")
    torch.cuda.synchronize()
    return d_moves.cpu().numpy(), d_draws.cpu().numpy().view(np.uint32)


def knowledge_scores(states, players):
    """KnowledgeSearch.score_move(board, (r, c), player) for every cell of every
    state (gz_knowledge_scores): float64 [n, 225], -1e9 at occupied cells."""
    lib = require_gpu()
    states = np.ascontiguousarray(states, dtype=STATE_DTYPE)
    n = len(states)
    d_states = to_dev(states)
    d_pl = torch.as_tensor(np.asarray(players, np.int32)).cuda()
    d_sc = torch.empty(max(1, n) * 225, dtype=torch.float64, device="cuda")
    _lib.check(lib.gz_knowledge_scores(ptr(d_states), ptr(d_pl), n, ptr(d_sc), stream()), "gz_knowledge_scores")
    torch.cuda.synchronize()
    return d_sc[: n * 225].cpu().numpy().reshape(n, 225)
