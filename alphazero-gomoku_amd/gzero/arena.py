"""The PUCT arena: two networks play each other in one device-side match
(gz_puct_match_run, include/gzero.h).

Every slot plays one game.  Side A plays black in game g iff ((g ^ a_black_parity) & 1)
== 0, and the side that moves at a search's root evaluates every leaf of that search, so
each player searches with its own network and precision.  Nothing but the per-step
counters is read back while a match runs.
"""
import ctypes
import math

import numpy as np
import torch

from . import _lib
from .boards import RECORD_DTYPE, STATE_DTYPE
from .device import PVWeights, ptr, puct_params, puct_sym_bytes, require_gpu, stream
from .selfplay import COUNTER_DTYPE

TALLY_FIELDS = ("games", "a_wins", "b_wins", "draws", "a_wins_black", "a_wins_white", "b_wins_black",
                "b_wins_white", "plies")
_SLOT_GAME_ID = 64  # SlotHeader.game_id (csrc/gz_search.h): byte offset in a slot
_UNPLAYED = 2       # d_result of a game that has not finished


def wilson(score, n, z=1.959963984540054):
    """The Wilson score interval (95 % by default) of a proportion score / n: (low, high)."""
    if n <= 0:
        return (0.0, 1.0)
    p = score / n
    d = 1.0 + z * z / n
    mid = (p + z * z / (2.0 * n)) / d
    half = z * math.sqrt(p * (1.0 - p) / n + z * z / (4.0 * n * n)) / d
    return (max(0.0, mid - half), min(1.0, mid + half))


class PuctMatch:
    """``games`` slots, the workspace, the records, the visit rows and the tally of one match.

    weights_a / weights_b: PVWeights (blob and precision) of side A and side B.  Game i has
    the id game_id_base + i * game_id_stride.  :meth:`step` plays plies and tallies the games
    they finished; :meth:`run` steps (compacting the live slots to the front after every
    step unless compact=False) until every game is over.  dirichlet_alpha: root noise as in
    SelfPlayEngine (None: none).  leaf_symmetry: every leaf under a board symmetry picked by
    (seed, position), the same for both sides (GZ_PUCT_LEAF_SYM; default off)."""

    def __init__(self, weights_a, weights_b, games, num_simulations=200, c_puct=1.6, temp_plies=8, seed=0,
                 dirichlet_alpha=None, noise_eps=0.25, game_id_base=0, a_black_parity=0, game_id_stride=1,
                 compact=True, leaf_symmetry=False):
        self.lib = require_gpu()
        if not isinstance(weights_a, PVWeights) or not isinstance(weights_b, PVWeights):
            raise ValueError("a match needs two PVWeights")
        self.n_slots = int(games)
        if self.n_slots < 1:
            raise ValueError("a match needs at least one game")
        self.stride = int(game_id_stride)
        if self.stride < 1:
            raise ValueError("game_id_stride must be at least 1")
        self.parity = int(a_black_parity)
        self.base = int(game_id_base)
        self.weights = (weights_a, weights_b)
        # (the precision field of the shared params is not read by a match)
        self.search = puct_params(num_simulations, c_puct, temp_plies, seed, "f16x3", dirichlet_alpha, noise_eps,
                                  leaf_symmetry=leaf_symmetry)
        S = self.S = self.search.num_simulations
        self.params = _lib.PuctMatchParams(
            ctypes.cast(ctypes.pointer(self.search), ctypes.c_void_p),
            (ctypes.c_void_p * 2)(weights_a.tensor.data_ptr(), weights_b.tensor.data_ptr()),
            (ctypes.c_int32 * 2)(weights_a.mode, weights_b.mode), self.parity, 0)
        n = self.n_slots
        self.n_active = n
        self.compacting = bool(compact)
        # (gz_selfplay_init writes every slot's whole header; records and visit rows at or past
        # the counters' record count are not written and not read)
        self.d_slots = torch.empty(n * self.lib.gz_slot_bytes(S), dtype=torch.uint8, device="cuda")
        self.d_ws = torch.empty(self.lib.gz_puct_match_workspace_bytes(n, S) + puct_sym_bytes(self.lib, n, self.search),
                                dtype=torch.uint8, device="cuda")
        self.record_cap = n * _lib.GZ_MAX_GAME_PLIES  # one game per slot
        self.d_records = torch.empty(self.record_cap * RECORD_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        self.d_visits = torch.empty(self.record_cap * 225, dtype=torch.int16, device="cuda")
        # in/out (gzero.h: "d_counters is added to, never cleared: the caller zeroes it")
        self.d_counters = torch.zeros(COUNTER_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        # in/out (gzero.h: "the caller zeroes it once per match")
        self.d_tally = torch.zeros(len(TALLY_FIELDS), dtype=torch.int64, device="cuda")
        self.span = (n - 1) * self.stride + 1
        # in/out (gzero.h: "games not in d_records are left alone")
        self.d_result = torch.full((self.span,), _UNPLAYED, dtype=torch.int8, device="cuda")
        self.d_order = torch.empty(n, dtype=torch.int32, device="cuda")
        self.d_n_active = torch.full((1,), n, dtype=torch.int32, device="cuda")
        self.d_compact_ws = torch.empty(self.lib.gz_selfplay_puct_compact_workspace_bytes(n), dtype=torch.uint8,
                                        device="cuda")
        # slot s plays the one game base + s * stride: the next id of every slot is past the end
        end = self.base + n * self.stride
        _lib.check(self.lib.gz_selfplay_init(ptr(self.d_slots), n, S, self.base, n * self.stride, stream()),
                   "gz_selfplay_init")
        if self.stride != 1:
            ids = self.base + torch.arange(n, dtype=torch.int64, device="cuda") * self.stride
            self.d_slots.view(torch.int64).view(n, -1)[:, _SLOT_GAME_ID // 8] = ids
        _lib.check(self.lib.gz_selfplay_set_game_end(ptr(self.d_slots), n, end, stream()), "gz_selfplay_set_game_end")
        self.games_done = 0
        self.moves_played = 0
        self.steps = 0
        self.last_count = 0
        self._recs, self._vis = [], []

    # ---- launches
    def launch(self, n_plies=1):
        """n_plies plies of the first n_active slots (asynchronous); the counters are the step's."""
        self.d_counters.zero_()
        if self.n_active == 0:
            return
        _lib.check(self.lib.gz_puct_match_run(ptr(self.d_slots), self.n_slots, self.n_active,
                                              ctypes.byref(self.params), ptr(self.d_ws), int(n_plies),
                                              ptr(self.d_records), self.record_cap, ptr(self.d_visits),
                                              ptr(self.d_counters), stream()), "gz_puct_match_run")

    def advance(self, n_plies):
        """Benchmark burn-in (as SelfPlayEngine.advance): n_plies plies at 8 simulations
        without root noise (leaf_symmetry stays), in the match's own workspace.  Games that end
        here are neither tallied nor kept."""
        p = _lib.PuctParams.from_buffer_copy(self.search)
        p.flags &= _lib.GZ_PUCT_LEAF_SYM
        p.num_simulations = min(8, p.num_simulations)
        mp = _lib.PuctMatchParams.from_buffer_copy(self.params)
        mp.search = ctypes.cast(ctypes.pointer(p), ctypes.c_void_p)
        for _ in range(int(n_plies)):
            self.d_counters.zero_()
            _lib.check(self.lib.gz_puct_match_run(ptr(self.d_slots), self.n_slots, self.n_active, ctypes.byref(mp),
                                                  ptr(self.d_ws), 1, ptr(self.d_records), self.record_cap,
                                                  ptr(self.d_visits), ptr(self.d_counters), stream()),
                       "gz_puct_match_run")

    def compact(self):
        """gz_selfplay_puct_compact on the match workspace (move_trees = 0: every tree is
        rebuilt each ply); returns the device int32 [1] active count."""
        if self.n_active > 0:
            _lib.check(self.lib.gz_selfplay_puct_compact(ptr(self.d_slots), self.n_slots, self.n_active, self.S, 0, 0,
                                                         ptr(self.d_ws), ptr(self.d_order), ptr(self.d_n_active),
                                                         ptr(self.d_compact_ws), stream()),
                       "gz_selfplay_puct_compact")
        return self.d_n_active

    def step(self, n_plies=1):
        """Play n_plies plies, compact (when compacting), read the step's counters and the
        active count back in one copy, tally the games that finished and keep their
        records and visit rows.  Returns the number of records of the step."""
        self.launch(n_plies)
        parts = [self.d_counters.view(torch.int64)]
        if self.compacting and self.n_active > 0:
            parts.append(self.compact().to(torch.int64))
        c = torch.cat(parts).cpu().numpy()
        if len(c) > 5:
            self.n_active = int(c[5])
        head = c[:2].view(np.int32)  # records, leaves, records_dropped, leaves_dropped
        if head[2]:
            raise RuntimeError(f"PuctMatch: {int(head[2])} records dropped")
        self.moves_played += int(c[2])
        self.games_done += int(c[3])
        self.steps += 1
        n = self.last_count = min(int(head[0]), self.record_cap)
        if n:
            _lib.check(self.lib.gz_puct_match_results(ptr(self.d_records), n, self.parity, self.base, self.span,
                                                      ptr(self.d_tally), ptr(self.d_result), stream()),
                       "gz_puct_match_results")
            self._recs.append(self.d_records[: n * RECORD_DTYPE.itemsize].clone())
            self._vis.append(self.d_visits[: n * 225].clone())
        if not self.compacting and self.games_done >= self.n_slots:
            self.n_active = 0
        return n

    def finished(self):
        return self.games_done >= self.n_slots

    def run(self, plies_per_step=1):
        """Steps until every game is over; returns :meth:`tally`."""
        max_steps = _lib.GZ_MAX_GAME_PLIES // int(plies_per_step) + 2
        while not self.finished():
            if self.steps >= max_steps:
                raise RuntimeError(f"PuctMatch: {self.games_done} of {self.n_slots} games after {self.steps} steps")
            self.step(plies_per_step)
        return self.tally()

    # ---- host views (synchronising)
    def counters(self):
        return np.frombuffer(self.d_counters.cpu().numpy().tobytes(), COUNTER_DTYPE)[0]

    def tally(self):
        t = self.d_tally.cpu().numpy()
        return {k: int(t[i]) for i, k in enumerate(TALLY_FIELDS)}

    def results(self):
        """int8 per game in id order: +1 A won, -1 B won, 0 a draw, 2 not finished."""
        return self.d_result.cpu().numpy()[:: self.stride].copy()

    def step_records(self):
        """(records, visit rows uint16 [n, 225]) of the games that finished in the last step,
        as the engine wrote them."""
        n = self.last_count
        raw = self.d_records[: n * RECORD_DTYPE.itemsize].cpu().numpy()
        return (np.frombuffer(raw.tobytes(), RECORD_DTYPE),
                self.d_visits[: n * 225].cpu().numpy().view(np.uint16).reshape(n, 225))

    def records(self):
        """(records, visit rows) of every finished game so far, sorted by (game id, ply)."""
        if not self._recs:
            return np.zeros(0, RECORD_DTYPE), np.zeros((0, 225), np.uint16)
        recs = np.frombuffer(torch.cat(self._recs).cpu().numpy().tobytes(), RECORD_DTYPE)
        vis = torch.cat(self._vis).cpu().numpy().view(np.uint16).reshape(-1, 225)
        order = np.lexsort((recs["ply"], recs["game_id"]))
        return recs[order], vis[order]

    def boards(self):
        """(states, game ids) of every slot, in slot order (permuted by a compaction)."""
        out = torch.empty(self.n_slots * STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        gids = torch.empty(self.n_slots, dtype=torch.int64, device="cuda")
        _lib.check(self.lib.gz_selfplay_boards(ptr(self.d_slots), self.n_slots, self.S, ptr(out), ptr(gids),
                                               stream()), "gz_selfplay_boards")
        return np.frombuffer(out.cpu().numpy().tobytes(), STATE_DTYPE), gids.cpu().numpy()


def summarise(tally):
    """A tally as evaluate_model's keys (from A's side) plus the colour split, the plies
    and the 95 % Wilson interval of the score (wins + draws / 2) / games."""
    g = tally["games"]
    score = tally["a_wins"] + 0.5 * tally["draws"]
    lo, hi = wilson(score, g)
    return {"wins": tally["a_wins"], "losses": tally["b_wins"], "draws": tally["draws"],
            "win_rate": tally["a_wins"] / max(1, g), "games_played": g,
            "wins_black": tally["a_wins_black"], "wins_white": tally["a_wins_white"],
            "losses_black": tally["b_wins_white"], "losses_white": tally["b_wins_black"],
            "plies": tally["plies"], "score": score / max(1, g), "wilson95": (lo, hi)}


def play_match(model_a, model_b, games=64, num_simulations=200, c_puct=1.6, temp_plies=8, seed=0, precision_a=None,
               precision_b=None, dirichlet_alpha=None, noise_eps=0.25, game_id_base=0, return_games=False,
               a_black_parity=None, plies_per_step=1, leaf_symmetry=False):
    """A match of ``games`` games between two models (GomokuModel: the blobs are
    model.device_weights(precision), None = the model's own precision), colours alternating
    by game: A is black in the first game (a_black_parity None = game_id_base & 1).  Returns
    wins / losses / draws / win_rate from A's side (evaluate_model's keys), wins_black /
    wins_white / losses_black / losses_white (A's colour in those games), plies, score =
    (wins + draws / 2) / games and its 95 % Wilson interval; with return_games also
    "games": per game its id, moves, winner (1 / 2 / None) and color_a."""
    wa, wb = model_a.device_weights(precision_a), model_b.device_weights(precision_b)
    parity = int(game_id_base) & 1 if a_black_parity is None else int(a_black_parity)
    m = PuctMatch(wa, wb, games, num_simulations=num_simulations, c_puct=c_puct, temp_plies=temp_plies, seed=seed,
                  dirichlet_alpha=dirichlet_alpha, noise_eps=noise_eps, game_id_base=game_id_base,
                  a_black_parity=parity, leaf_symmetry=leaf_symmetry)
    out = summarise(m.run(plies_per_step))
    out["precisions"] = (wa.precision, wb.precision)
    if return_games:
        recs, _ = m.records()
        res = m.results()
        out["games"] = []
        for i in range(int(games)):
            gid = int(game_id_base) + i
            r = recs[recs["game_id"] == gid]
            color_a = 1 if ((gid ^ parity) & 1) == 0 else 2
            z = int(res[i])
            winner = None if z == 0 else (color_a if z > 0 else 3 - color_a)
            out["games"].append({"game_id": gid, "moves": [int(x) for x in r["move"]], "winner": winner,
                                 "color_a": color_a})
    return out
