"""Device-resident self-play collector: the batched form of
``training.play_one_game`` (training.py:141-218) over thousands of concurrent games.

One call of :meth:`SelfPlayEngine.step` advances every game slot by ``n_plies``
plies inside one kernel launch (one wavefront per game), then -- in
reference-work mode -- evaluates the policy-value network on every node the
searches created, exactly the ``GomokuModel.predict`` calls the reference makes
(``ai_agent.py:522-523``).  The forward's outputs are produced but, as in the
reference, never read by the search.  Finished games are appended as
(planes, move, player, z) records; slots restart with the next game id.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .boards import RECORD_DTYPE, STATE_DTYPE, words_to_cells
from .device import (GNWeights, PVWeights, ptr, puct_extra_bytes, puct_leaves, puct_params, require_gpu, search_params,
                     stream)

COUNTER_DTYPE = np.dtype([("records", "<i4"), ("leaves", "<i4"), ("records_dropped", "<i4"),
                          ("leaves_dropped", "<i4"), ("moves", "<i8"), ("games", "<i8"),
                          ("mcts_moves", "<i8")])


class SelfPlayEngine:
    def __init__(self, n_slots=4096, num_simulations=200, c_puct=1.6, exploration=0.05, beta=0.2,
                 seed=0, max_depth=100, pv_weights=None, plies_per_step=1, game_id_base=0,
                 game_id_stride=None, planner_steps=0, planner_difficulty="medium", gn_weights=None,
                 pv_mode="full", game_id_end=None, search="reference", temp_plies=12, tree_reuse=False,
                 rounds_per_step=None, dirichlet_alpha=None, noise_eps=0.25, leaves_per_round=1,
                 compact_slots=False, fast_simulations=None, full_prob=0.25, leaf_symmetry=False,
                 forced_playouts=None, gumbel_considered=None, c_visit=50.0, c_scale=0.5, gumbel_scale=1.0):
        """search: "reference" (default) = the reference's search, in which the network's
        outputs are computed and never read; "puct" = the network-guided search
        (gz_selfplay_puct_run): the priors steer selection, the value head replaces the
        rollout, plies below temp_plies sample the move from the root visit counts and
        the later ones take the most visited cell.  "puct" needs pv_weights (its
        precision is the forward's) and planner_steps == 0, and ignores beta,
        exploration, max_depth and pv_mode.  Every record then has a visit row
        (:meth:`visits`), the policy target; records["move"] is still the move played.
        tree_reuse (search="puct" only): the subtree under the move played is the next
        ply's tree and every slot keeps its own clock (gz_selfplay_puct_rounds): a
        search ends when its root has num_simulations + 1 visits, so a root that
        inherits v visits plays after num_simulations + 1 - v rounds, and every round is
        one forward in which every live slot has a leaf.  :meth:`step` then runs
        rounds_per_step rounds (default num_simulations + 1, the rounds of one lock-step
        ply), so the moves per step vary; a game's moves and visit rows do not depend on
        the slot count or on rounds_per_step.
        dirichlet_alpha (search="puct" only; default None = no noise): Dirichlet noise at
        every search root, prior' = (1 - noise_eps) prior + noise_eps Dir(dirichlet_alpha)
        over the empty cells, sampled on the device from the (seed, game id, ply) stream
        (GZ_PUCT_ROOT_NOISE, include/gzero.h), in lock-step and with tree_reuse alike:
        without it play from temp_plies on is a deterministic function of the position.
        leaves_per_round K (search="puct" only; default 1 = the unbatched search): leaf
        batching with virtual loss, K leaves per slot per round in one forward of
        n_slots K rows, about 1 + ceil(num_simulations / K) rounds per move instead of
        num_simulations + 1 (GZ_PUCT_LEAF_BATCH, include/gzero.h) -- for small n_slots,
        where a forward of a few boards leaves the chip idle.  The search then
        synchronises with the host once per block of rounds.  Not with tree_reuse.
        fast_simulations F (search="puct" only; default None = no cap): playout cap
        randomization (GZ_PUCT_PLAYOUT_CAP, include/gzero.h): every ply is a full search
        of num_simulations with probability full_prob, else a fast one of F simulations
        without root noise, decided from (seed, game id, ply).  Every ply is recorded;
        gzero.device.cap_full tells which records were full plies, the ones to train on.
        With tree_reuse a move then takes B + 1 - v rounds (at least one), B its ply's
        budget; the lock-step engine accepts the cap and gains nothing (every ply costs
        num_simulations + 1 rounds).  rounds_per_step keeps its default.  Not with
        leaves_per_round > 1.
        leaf_symmetry (search="puct" only; default False): every leaf is evaluated under one
        of the 8 board symmetries, picked by (seed, position), and its prior mapped back
        (GZ_PUCT_LEAF_SYM, include/gzero.h), so the network's orientation bias averages out
        over a search.  Lock-step and tree_reuse alike, with every other option; the burn-in
        of :meth:`advance` keeps it.
        forced_playouts k (search="puct" only; default None = the flag clear): forced playouts
        and policy-target pruning (GZ_PUCT_FORCED_PLAYOUTS, include/gzero.h; KataGo's k = 2):
        at a full-budget root a visited child gets at least sqrt(k prior visits) playouts, so
        a noised move is examined and not just tried once, and the visit row that becomes the
        policy target gives back the forced playouts the move did not earn by PUCT.  The move
        played comes from the raw counts; rows no longer sum to num_simulations.  Lock-step
        and tree_reuse alike; fast plies of a playout cap neither force nor prune; the
        burn-in of :meth:`advance` does not force.  Not with leaves_per_round > 1.
        gumbel_considered m (search="puct" only; default None = the flag clear): the Gumbel root
        with sequential halving (GZ_PUCT_GUMBEL, include/gzero.h; Danihelka et al. 2022), the
        search for budgets of 16..32 simulations: m root moves sampled without replacement, the
        budget halved among them, the move from g + logit + sigma(q) and, as the policy target,
        the improved policy softmax(logit + sigma(completed q)) as a row scaled to 32767 in
        place of the visit counts (c_visit, c_scale, gumbel_scale: puct_params).  temp_plies is
        not read and no main-stream draw is made.  Lock-step only (tree_reuse raises), with
        leaf_symmetry and compact_slots; not with dirichlet_alpha, leaves_per_round > 1,
        fast_simulations or forced_playouts; the burn-in of :meth:`advance` is plain PUCT.
        game_id_end: a slot whose next game id would be >= game_id_end goes idle
        instead of restarting (gz_selfplay_set_game_end; default: continuous refill);
        :meth:`compact` then moves the active slots to the front so that only those run.
        compact_slots (search="puct" with a game_id_end only): :meth:`compact` works on this
        PUCT engine (gz_selfplay_puct_compact, in place): active slots from the tail fill the
        idle places in front, their pending visit rows and, with tree_reuse, their trees
        moving with them.  The slot order is not preserved: after a compaction
        :meth:`draws`, :meth:`boards` and every other per-slot view are permuted
        (:attr:`d_order` holds the last permutation); a game's moves, visit rows and z are
        the same with and without it.
        planner_steps > 0: BG-planner rollout plies (config 4); gn_weights = the
        planner's GraphNet/DQN blob (gzero.planner_nets) or a GNWeights.
        pv_mode: "full" = one full forward per node (gz_pv_forward); "tree" = the
        incremental forward (gz_pv_forward_tree, f16x3 only): a root's children as the
        root's pre-BN accumulators plus the convolution of their input differences
        (within 2e-5 of the full forward), its grandchildren the same delta of their
        parent; roots and other nodes bit-identical to "full"."""
        if search not in ("reference", "puct"):
            raise ValueError(f"search must be 'reference' or 'puct', not {search!r}")
        self.search = search
        self.tree_reuse = bool(tree_reuse)
        if self.tree_reuse and search != "puct":
            raise ValueError("tree_reuse needs search='puct'")
        if dirichlet_alpha is not None and search != "puct":
            raise ValueError("dirichlet_alpha needs search='puct'")
        self.leaves_per_round = int(leaves_per_round)
        if self.leaves_per_round != 1 and search != "puct":
            raise ValueError("leaves_per_round needs search='puct'")
        if self.leaves_per_round > 1 and self.tree_reuse:
            raise ValueError("leaves_per_round > 1 is not supported with tree_reuse")
        if fast_simulations is not None:
            if search != "puct":
                raise ValueError("fast_simulations needs search='puct'")
            if self.leaves_per_round > 1:
                raise ValueError("fast_simulations (the playout cap) is not supported with leaves_per_round > 1")
        self.leaf_symmetry = bool(leaf_symmetry)
        if self.leaf_symmetry and search != "puct":
            raise ValueError("leaf_symmetry needs search='puct'")
        if forced_playouts is not None:
            if search != "puct":
                raise ValueError("forced_playouts needs search='puct'")
            if self.leaves_per_round > 1:
                raise ValueError("forced_playouts is not supported with leaves_per_round > 1")
        if gumbel_considered is not None:
            if search != "puct":
                raise ValueError("gumbel_considered needs search='puct'")
            if self.tree_reuse:
                raise ValueError("gumbel_considered is not supported with tree_reuse")
        if search == "puct":
            if pv_weights is None:
                raise ValueError("search='puct' needs pv_weights (the network guides the search)")
            if int(planner_steps) != 0:
                raise ValueError("search='puct' has no rollouts: planner_steps must be 0")
        self.compact_slots = bool(compact_slots)
        if self.compact_slots and (search != "puct" or game_id_end is None):
            raise ValueError("compact_slots needs search='puct' and a game_id_end")
        self.lib = require_gpu()
        self.n_slots = int(n_slots)
        self.n_active = self.n_slots  # the slots the launches run (the first n_active)
        self.plies_per_step = int(plies_per_step)
        # (the PUCT search evaluates its own leaves: nothing is gathered for a forward afterwards)
        self.gather = pv_weights is not None and search != "puct"
        self.planner_steps = int(planner_steps)
        self.params = search_params(num_simulations, c_puct, exploration, beta, seed, max_depth,
                                    self.planner_steps, self.gather)
        if self.planner_steps:
            if gn_weights is None:
                raise ValueError("planner_steps > 0 needs gn_weights (the planner's GraphNet/DQN)")
            self.gn_weights = gn_weights if isinstance(gn_weights, GNWeights) else GNWeights(gn_weights)
            self.pparams = _lib.planner_params(planner_difficulty)
            self.d_plan_ws = torch.empty(self.lib.gz_selfplay_plan_workspace_bytes(self.n_slots, num_simulations),
                                         dtype=torch.uint8, device="cuda")
            self.gn_stats(reset=True)
        self.pv_weights = pv_weights if (pv_weights is None or isinstance(pv_weights, PVWeights)) \
            else PVWeights(pv_weights)
        if pv_mode not in ("full", "tree"):
            raise ValueError(f"pv_mode must be 'full' or 'tree', not {pv_mode!r}")
        self.tree = pv_mode == "tree" and self.gather
        self.pv_mode = pv_mode if self.gather else "full"
        if self.tree and self.pv_weights.mode != _lib.GZ_PV_F16X3:
            raise ValueError(f"pv_mode={pv_mode!r} needs f16x3 weights")
        S = self.params.num_simulations
        slot_bytes = self.lib.gz_slot_bytes(S)
        # (gzero.h: "gz_selfplay_init writes the whole 128-byte header of every slot; the record
        # area behind it is written ply by ply before it is read")
        self.d_slots = torch.empty(self.n_slots * slot_bytes, dtype=torch.uint8, device="cuda")
        self.rounds_per_step = (S + 1 if rounds_per_step is None else int(rounds_per_step)) if self.tree_reuse else 0
        if self.tree_reuse and self.rounds_per_step < 1:
            raise ValueError("rounds_per_step must be at least 1")
        # a slot can finish one 200-ply game plus any games played inside a step (with
        # tree reuse: at most 199 earlier plies plus one per round)
        self.record_cap = self.n_slots * (_lib.GZ_MAX_GAME_PLIES +
                                          (self.rounds_per_step if self.tree_reuse else self.plies_per_step))
        self.d_records = torch.empty(self.record_cap * RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        # in/out (gzero.h: "d_counters is added to, never cleared: the caller zeroes it")
        self.d_counters = torch.zeros(COUNTER_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        self.puct = self.d_puct_ws = self.d_visits = None
        if search == "puct":
            self.puct = puct_params(S, c_puct, temp_plies, seed, self.pv_weights.precision, dirichlet_alpha,
                                    noise_eps, self.leaves_per_round, fast_simulations, full_prob,
                                    self.leaf_symmetry, forced_playouts, gumbel_considered, c_visit, c_scale,
                                    gumbel_scale)
            K = puct_leaves(self.puct)
            nbytes = self.lib.gz_selfplay_puct_batch_workspace_bytes(self.n_slots, S, K) if K else \
                self.lib.gz_selfplay_puct_workspace_bytes(self.n_slots, S)
            # (the transform of every round row and the Gumbel root's region, behind the flag-clear
            # workspace)
            nbytes = puct_extra_bytes(self.lib, nbytes, self.n_slots * max(1, K), self.n_slots, self.puct)
            self.d_puct_ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            # uint16 [record_cap][225] visit rows, aligned with d_records (int16 storage: torch
            # has no uint16 arithmetic; a count is at most GZ_MAX_SIMULATIONS)
            self.d_visits = torch.empty(self.record_cap * 225, dtype=torch.int16, device="cuda")
            if self.tree_reuse:
                self._puct_reset()
        self.leaf_cap = self.n_slots * self.plies_per_step * (S + 1) if self.gather else 0
        if self.gather:
            self.d_leaves = torch.empty(self.leaf_cap * 16, dtype=torch.int32, device="cuda")
            self.d_logits = torch.empty(self.leaf_cap * 225, dtype=torch.float32, device="cuda")
            self.d_value = torch.empty(self.leaf_cap, dtype=torch.float32, device="cuda")
            self.d_probs = torch.empty(self.leaf_cap * 225, dtype=torch.float32, device="cuda")
            # MCTSNode.prior_prob of every node (ai_agent.py:522-523,564-582), dense float64
            self.d_prior = torch.empty(self.leaf_cap * 225, dtype=torch.float64, device="cuda")
        else:
            self.d_leaves = self.d_logits = self.d_value = self.d_probs = self.d_prior = None
        self.d_meta = self.d_tree_ws = None
        if self.tree:
            self.d_meta = torch.empty(self.leaf_cap, dtype=torch.int32, device="cuda")
            # one root per slot per ply, and a quarter more: the patch slots (11.9 per root
            # slot) are one pool, and a ply-step needs about 13.4 per root that moves
            roots = self.n_slots * self.plies_per_step
            self.root_cap = roots + (roots + 3) // 4
            self.d_tree_ws = torch.empty(self.lib.gz_pv_tree_workspace_bytes(self.leaf_cap, self.root_cap),
                                         dtype=torch.uint8, device="cuda")
        base = int(game_id_base)
        stride = self.n_slots if game_id_stride is None else int(game_id_stride)
        _lib.check(self.lib.gz_selfplay_init(ptr(self.d_slots), self.n_slots, S, base, stride, stream()),
                   "gz_selfplay_init")
        self.d_slots_alt = self.d_compact_ws = self.d_n_active = None
        if game_id_end is not None:
            _lib.check(self.lib.gz_selfplay_set_game_end(ptr(self.d_slots), self.n_slots, int(game_id_end), stream()),
                       "gz_selfplay_set_game_end")
            self.d_n_active = torch.empty(1, dtype=torch.int32, device="cuda")
        self.d_order = None
        if self.compact_slots:  # in place: no second slot buffer
            self.d_compact_ws = torch.empty(self.lib.gz_selfplay_puct_compact_workspace_bytes(self.n_slots),
                                            dtype=torch.uint8, device="cuda")
            self.d_order = torch.empty(self.n_slots, dtype=torch.int32, device="cuda")
        elif game_id_end is not None:
            self.d_slots_alt = torch.empty_like(self.d_slots)
            self.d_compact_ws = torch.empty(self.lib.gz_selfplay_compact_workspace_bytes(self.n_slots),
                                            dtype=torch.uint8, device="cuda")

    def compact(self):
        """Launch gz_selfplay_compact: the active slots to the front of the slot buffer
        (the two buffers swap).  Returns the device int32 [1] active count; the caller
        sets :attr:`n_active` from it once read (the next launches run that many).
        On a PUCT engine built with compact_slots: gz_selfplay_puct_compact among the first
        :attr:`n_active` slots, in place -- the slots, their pending visit rows and (with
        tree_reuse) their trees; the slot order, and with it :meth:`draws` and
        :meth:`boards`, is permuted (d_order[:n_active]: the new index of each old slot)."""
        if self.compact_slots:
            if self.n_active > 0:
                _lib.check(self.lib.gz_selfplay_puct_compact(
                    ptr(self.d_slots), self.n_slots, self.n_active, self.puct.num_simulations, self.leaves_per_round,
                    1 if self.tree_reuse else 0, ptr(self.d_puct_ws), ptr(self.d_order), ptr(self.d_n_active),
                    ptr(self.d_compact_ws), stream()), "gz_selfplay_puct_compact")
            return self.d_n_active
        if self.search == "puct":
            # the pending visit rows live per slot in the workspace and have to move too
            raise ValueError("compact() on a PUCT engine needs compact_slots=True")
        if self.d_slots_alt is None:
            raise ValueError("compact() needs an engine built with game_id_end")
        _lib.check(self.lib.gz_selfplay_compact(ptr(self.d_slots), self.n_slots, ptr(self.d_slots_alt),
                                                ptr(self.d_n_active), ptr(self.d_compact_ws), stream()),
                   "gz_selfplay_compact")
        self.d_slots, self.d_slots_alt = self.d_slots_alt, self.d_slots
        return self.d_n_active

    # ---- launches (asynchronous, current torch stream)
    def launch_search(self, n_plies=None):
        n = self.plies_per_step if n_plies is None else int(n_plies)
        if n > self.plies_per_step and self.gather:
            raise ValueError("n_plies exceeds the leaf buffer sized for plies_per_step")
        self.d_counters.zero_()
        if self.n_active == 0:  # every game is done
            return
        if self.tree_reuse:
            # n_plies counts steps of rounds_per_step rounds here
            self._puct_rounds(self.rounds_per_step * (1 if n_plies is None else int(n_plies)))
            return
        if self.search == "puct":
            self._puct_run(self.puct, n)
            return
        if self.planner_steps:
            _lib.check(self.lib.gz_selfplay_plan_run(ptr(self.d_slots), self.n_active, ctypes.byref(self.params),
                                                     ctypes.byref(self.pparams), ptr(self.gn_weights.tensor),
                                                     ptr(self.d_plan_ws), n, ptr(self.d_records), self.record_cap,
                                                     ptr(self.d_leaves), self.leaf_cap, ptr(self.d_meta),
                                                     ptr(self.d_counters), stream()), "gz_selfplay_plan_run")
            return
        _lib.check(self.lib.gz_selfplay_run(ptr(self.d_slots), self.n_active, ctypes.byref(self.params), n,
                                            ptr(self.d_records), self.record_cap, ptr(self.d_leaves),
                                            self.leaf_cap, ptr(self.d_meta), ptr(self.d_counters), stream()),
                   "gz_selfplay_run")

    def _puct_run(self, p, n_plies):
        # (n_slots carved the workspace; the first n_active slots run)
        _lib.check(self.lib.gz_selfplay_puct_run_active(ptr(self.d_slots), self.n_slots, self.n_active,
                                                        ctypes.byref(p), ptr(self.pv_weights.tensor),
                                                        ptr(self.d_puct_ws), int(n_plies), ptr(self.d_records),
                                                        self.record_cap, ptr(self.d_visits), ptr(self.d_counters),
                                                        stream()), "gz_selfplay_puct_run_active")

    def _puct_rounds(self, n_rounds):
        _lib.check(self.lib.gz_selfplay_puct_rounds_active(ptr(self.d_slots), self.n_slots, self.n_active,
                                                           ctypes.byref(self.puct), ptr(self.pv_weights.tensor),
                                                           ptr(self.d_puct_ws), int(n_rounds), ptr(self.d_records),
                                                           self.record_cap, ptr(self.d_visits), ptr(self.d_counters),
                                                           stream()), "gz_selfplay_puct_rounds_active")

    def _puct_reset(self):
        _lib.check(self.lib.gz_selfplay_puct_reset(ptr(self.d_puct_ws), self.n_slots, self.puct.num_simulations,
                                                   stream()), "gz_selfplay_puct_reset")

    def gn_stats(self, reset=False, check=None):
        """Planner-net rows since the last reset: {"full", "incremental", "checked",
        "mismatched"} (gz_selfplay_plan_gn_stats; synchronises).  check=True/False
        turns GZ_FLAG_GN_CHECK (every incremental row re-run by the full forward and
        compared bitwise) on/off for the following searches."""
        if getattr(self, "d_slots_alt", None) is not None:
            # a compacting engine carves the planner workspace for n_active slots, so the
            # counters' place moves with it: they cannot be read at n_slots
            raise ValueError("gn_stats() is not available on an engine built with game_id_end (compaction)")
        if check is not None:
            f = self.params.flags & ~_lib.GZ_FLAG_GN_CHECK
            self.params.flags = f | (_lib.GZ_FLAG_GN_CHECK if check else 0)
        out = (ctypes.c_int64 * 4)()
        _lib.check(self.lib.gz_selfplay_plan_gn_stats(ptr(self.d_plan_ws), self.n_slots, self.params.num_simulations,
                                                      out, 1 if reset else 0, stream()), "gz_selfplay_plan_gn_stats")
        return {"full": out[0], "incremental": out[1], "checked": out[2], "mismatched": out[3]}

    def advance(self, n_plies):
        """Play n_plies plies on every slot without gathering leaves for the PV forward
        (the moves are the same either way: the search never reads the priors,
        ai_agent.py:523).  Used to bring the slots to a steady-state mix of game plies
        (continuous refill) before a measurement; records of games finished here are
        not kept.  On a planner engine (config 4) the burn-in plies are searched without
        planner plies (the planner pipeline needs the GN forward per ply): the slots
        reach a steady-state mix of positions, and the measured plies are planner plies.
        On a PUCT engine the burn-in plies are PUCT plies at 8 simulations (every ply
        needs its visit row) without root noise, in the engine's own workspace; with tree_reuse they are
        lock-step plies too, and the trees are reset afterwards (the next round begins
        every slot with a fresh root)."""
        if self.search == "puct":
            # (the 32 bytes of the base struct: the burn-in has no root noise, no playout cap and
            # one leaf per round, so the flags that would make the library read past the copy are
            # cleared; leaf_symmetry has no struct of its own and stays: the burn-in is a search too)
            p = _lib.PuctParams.from_buffer_copy(self.puct)
            p.flags &= ~(_lib.GZ_PUCT_ROOT_NOISE | _lib.GZ_PUCT_LEAF_BATCH | _lib.GZ_PUCT_PLAYOUT_CAP |
                         _lib.GZ_PUCT_FORCED_PLAYOUTS | _lib.GZ_PUCT_GUMBEL)
            p.num_simulations = min(8, p.num_simulations)
            for _ in range(int(n_plies) if self.n_active > 0 else 0):
                self.d_counters.zero_()
                self._puct_run(p, 1)
            if self.tree_reuse:
                self._puct_reset()
            return
        p = _lib.SearchParams.from_buffer_copy(self.params)
        p.flags = 0
        p.planner_steps = 0
        for _ in range(int(n_plies)):
            self.d_counters.zero_()
            _lib.check(self.lib.gz_selfplay_run(ptr(self.d_slots), self.n_slots, ctypes.byref(p), 1,
                                                ptr(self.d_records), self.record_cap, None, 0, None,
                                                ptr(self.d_counters), stream()), "gz_selfplay_run")

    def launch_pv(self):
        if not self.gather or self.n_active == 0:
            return
        d_count = self.d_counters[4:8]  # counters.leaves
        if self.tree:
            _lib.check(self.lib.gz_pv_forward_tree(ptr(self.pv_weights.tensor), ptr(self.d_leaves),
                                                   ptr(self.d_meta), self.leaf_cap, ptr(d_count), self.root_cap,
                                                   ptr(self.d_logits), ptr(self.d_value), ptr(self.d_probs),
                                                   ptr(self.d_prior), ptr(self.d_tree_ws), stream()),
                       "gz_pv_forward_tree")
            return
        _lib.check(self.lib.gz_pv_forward(ptr(self.pv_weights.tensor), ptr(self.d_leaves), self.leaf_cap,
                                          ptr(d_count), ptr(self.d_logits), ptr(self.d_value),
                                          ptr(self.d_probs), ptr(self.d_prior),
                                          ptr(self.pv_weights.workspace_for(self.leaf_cap)),
                                          self.pv_weights.mode, stream()), "gz_pv_forward")

    def step(self, n_plies=None):
        self.launch_search(n_plies)
        self.launch_pv()

    def tree_stats(self):
        """List sizes of the last tree forward: roots seen, roots with maps,
        incremental root children, full-forward boards, incremental grandchildren,
        patch slots claimed (synchronising)."""
        out = torch.empty(6, dtype=torch.int32, device="cuda")
        _lib.check(self.lib.gz_pv_tree_stats(ptr(self.d_tree_ws), self.leaf_cap, ptr(out), stream()),
                   "gz_pv_tree_stats")
        return [int(x) for x in out.cpu()]

    def tree_exec_flops(self):
        """(executed MFMA FLOP of the last tree forward, its node count): roots and
        deeper nodes run the full forward, a root child or grandchild the row tiles
        of its windows (csrc/gz_pvinc.hip).  Reads the leaves and tags (synchronising)."""
        n = min(int(self.counters()["leaves"]), self.leaf_cap)
        rows = self.d_leaves[: n * 16].cpu().numpy().view(np.uint32).reshape(n, 16)
        meta = self.d_meta[:n].cpu().numpy()
        return tree_exec_flops(rows, meta), n

    # ---- host views (synchronising)
    def counters(self):
        return np.frombuffer(self.d_counters.cpu().numpy().tobytes(), COUNTER_DTYPE)[0]

    def records(self):
        """Records of the games that finished during the last step."""
        c = self.counters()
        n = min(int(c["records"]), self.record_cap)
        raw = self.d_records[: n * RECORD_DTYPE.itemsize].cpu().numpy()
        return np.frombuffer(raw.tobytes(), RECORD_DTYPE)

    def records_device(self):
        """(device uint8 tensor of records, count) without copying to the host."""
        n = min(int(self.counters()["records"]), self.record_cap)
        return self.d_records[: n * RECORD_DTYPE.itemsize], n

    def visits_device(self):
        """(device int16 tensor [count, 225] of root visit counts, count): row i belongs to
        record i of :meth:`records_device` (PUCT engines only)."""
        if self.search != "puct":
            raise ValueError("visits are recorded by search='puct' engines only")
        n = min(int(self.counters()["records"]), self.record_cap)
        return self.d_visits[: n * 225].view(n, 225), n

    def visits(self):
        """uint16 [count, 225]: the root visit counts of the search behind each record of
        :meth:`records` (the policy target; zero at occupied cells, summing to
        num_simulations)."""
        d, _ = self.visits_device()
        return d.cpu().numpy().view(np.uint16)

    def boards(self):
        """(states, game ids) of every slot, in slot order (permuted by a compaction)."""
        out = torch.empty(self.n_slots * STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        gids = torch.empty(self.n_slots, dtype=torch.int64, device="cuda")
        _lib.check(self.lib.gz_selfplay_boards(ptr(self.d_slots), self.n_slots, self.params.num_simulations,
                                               ptr(out), ptr(gids), stream()), "gz_selfplay_boards")
        return np.frombuffer(out.cpu().numpy().tobytes(), STATE_DTYPE), gids.cpu().numpy()


    def draws(self):
        """int64 [n_slots, 3]: (predict calls, main-stream RNG draws, simulation-stream
        RNG draws) summed over every search each slot ran since the engine was created
        (gz_selfplay_draws).  The totals travel with the slot buffers: after a compaction
        the rows are permuted (and, in the default mode, the active slots' come first)."""
        out = torch.empty(self.n_slots * 3, dtype=torch.int64, device="cuda")
        _lib.check(self.lib.gz_selfplay_draws(ptr(self.d_slots), self.n_slots, ptr(out), stream()),
                   "gz_selfplay_draws")
        return out.cpu().numpy().reshape(self.n_slots, 3)


def records_to_games(recs):
    """Group records by game id -> {game_id: dict(moves, players, z, cells)} (ply order)."""
    out = {}
    for gid in np.unique(recs["game_id"]):
        r = recs[recs["game_id"] == gid]
        r = r[np.argsort(r["ply"])]
        out[int(gid)] = {"moves": [int(x) for x in r["move"]], "players": [int(x) for x in r["player"]],
                         "z": [int(x) for x in r["z"]], "cells": words_to_cells(r["black"], r["white"])}
    return out


def records_to_replay(recs):
    """SimpleReplay fields (training.py:77-97): states float32 [n,3,15,15], move
    indices, players, outcomes."""
    cells = words_to_cells(recs["black"], recs["white"]).reshape(-1, 15, 15)
    planes = np.stack([(cells == 1), (cells == 2), (cells == 0)], axis=1).astype(np.float32)
    return planes, recs["move"].astype(np.int64), recs["player"].astype(np.int64), recs["z"].astype(np.int64)


PV_FLOP_FULL = 2 * 133690114  # one full forward (gzero.weights.PV_MACS)


def _window_rows(rc, r):
    lo = np.maximum(rc - r, 0)
    hi = np.minimum(rc + r, 14)
    return hi - lo + 1


def tree_exec_flops(rows, meta):
    """MFMA FLOP the tree forward executes for leaves `rows` ([n,16] uint32) tagged
    `meta`: 2 x (MACs of every 16-row tile it runs), fp32-equivalent like the full
    forward's 267.38 MFLOP.  A tagged node (meta >= 0: a root child or a child of
    one; assumes no map / patch slot ran out) whose stone is at (r, c) runs, per residual conv L = 1..4
    (window radius L + 1), ceil(rows_L / 16) tiles of 16 positions x 128 channels x
    1152, one conv0 tile, the 1x1 heads at radius 5 and the FC heads."""
    meta = np.asarray(meta)
    kids = np.flatnonzero(meta >= 0)
    full = len(meta) - len(kids)
    if len(kids) == 0:
        return float(full * PV_FLOP_FULL)
    diff = rows[kids] ^ rows[meta[kids]]
    both = diff[:, :8] | diff[:, 8:]
    word = np.argmax(both != 0, axis=1)
    bitv = both[np.arange(len(kids)), word]
    bit = word * 32 + np.log2(bitv.astype(np.float64)).astype(np.int64)
    r, c = bit // 16, bit % 16
    macs = np.zeros(len(kids), np.float64)
    for L in range(1, 5):
        n_rows = _window_rows(r, L + 1) * _window_rows(c, L + 1)
        macs += np.ceil(n_rows / 16.0) * 16 * 128 * 1152
    n4 = _window_rows(r, 5) * _window_rows(c, 5)
    macs += 16 * 128 * 27 + n4 * 128 * 3 + 450 * 225 + 225 * 64 + 64
    return float(full * PV_FLOP_FULL + 2.0 * macs.sum())
