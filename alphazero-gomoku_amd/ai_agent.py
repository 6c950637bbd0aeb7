"""Drop-in ``ai_agent`` module (reference: ai_agent.py:23-623).

``AlphaZeroGomokuAI.get_move`` runs the reference's search -- opening book,
MCTS with UCT + beta*tanh(pattern/1e4), heuristic rollouts, exploration -- as
one wavefront on the MI355X (``gz_search``), and evaluates the policy-value
network on every node the search creates exactly as the reference does
(``ai_agent.py:522-523``; the result is not read by the search there either).

Randomness: the reference draws from the global ``random`` module (OS-seeded,
irreproducible).  Here every draw comes from counter-based streams keyed by
(``seed``, ``game_id``, ply, simulation) (gzero/rng.py); ``seed`` defaults to
a fresh random value, so unseeded AIs are as random as the reference's while a
fixed (seed, game_id) reproduces a game exactly, on any number of GPUs.

With ``planner_steps > 0`` (the reference's default, 5) every rollout starts
with that many BG-planner plies (ai_agent.py:265-274): the search runs as the
batched pipeline of ``gz_plan_search`` with the AI's ``bg_planner`` nets.
``search="puct"`` (opt-in; the default ``"reference"`` is everything above) runs
the network-guided PUCT search of ``gz_puct_search`` on every ply instead: the
model's priors steer selection and its value head replaces the rollout.  It has no
opening book and no exploration move, ignores ``beta`` and ``planner_steps``, samples
the move from the visit counts below ``temp_plies`` plies (default 0: always the most
visited cell) and sets ``last_search_visits`` / ``last_root_value``.
``leaves_per_round=K`` (default 1) evaluates K leaves per board per round with virtual
loss (``device.puct_params``): a move of one board then takes about ``1 + S/K``
forwards instead of ``S + 1``.  ``leaf_symmetry=True`` (default off) evaluates every
leaf under one of the 8 board symmetries, picked by (seed, position).  Play (here and in
the arena) is always noise-free: the Dirichlet noise at the search root
(``SelfPlayEngine(dirichlet_alpha=...)``) is self-play exploration only.
``time_limit`` is accepted for compatibility; the GPU completes every
simulation, so the reference's wall-clock cut-off (ai_agent.py:183-189) never
applies.
"""
import logging
import random
import time
from typing import List, Optional, Tuple

import numpy as np

from bg_planner import BGPlannerAI
from gomoku_board import GomokuBoard
from neural_network import GomokuModel
from gzero import _lib, device


class AlphaZeroGomokuAI:
    def __init__(self, player: int, difficulty: str = "medium", model_path: Optional[str] = None,
                 device: Optional[str] = None, beta: float = 0.2, planner_steps: int = 5,
                 time_limit: float = 5.0, time_reward_factor: float = 0.1, seed: Optional[int] = None,
                 game_id: int = 0, compute_priors: bool = True, search: str = "reference",
                 temp_plies: int = 0, leaves_per_round: int = 1, leaf_symmetry: bool = False):
        if search not in ("reference", "puct"):
            raise ValueError(f"search must be 'reference' or 'puct', not {search!r}")
        self.search = search
        self.temp_plies = int(temp_plies)
        self.leaves_per_round = int(leaves_per_round)
        if self.leaves_per_round != 1 and search != "puct":
            raise ValueError("leaves_per_round needs search='puct'")
        self.leaf_symmetry = bool(leaf_symmetry)
        if self.leaf_symmetry and search != "puct":
            raise ValueError("leaf_symmetry needs search='puct'")
        self.last_search_visits = None  # puct: int32 [n, 225] root visit counts of the last call
        self.last_root_value = None     # puct: the roots' mean value for the side to move
        self.player = player
        self.difficulty = difficulty
        self.name = f"AlphaZero_{difficulty}"
        self.device = device or "cpu"
        self.beta = float(beta)
        self.planner_steps = int(max(0, planner_steps))
        self.time_limit = float(time_limit)
        self.time_reward_factor = float(time_reward_factor)
        self.logger = logging.getLogger(__name__)
        self.model = GomokuModel(model_path=model_path, device=self.device)
        self.bg_planner = BGPlannerAI(player=self.player, difficulty=self.difficulty, device="cpu")
        # live knobs of the reference's table (ai_agent.py:65-90); bg_weight and
        # planning_steps are kept but, as in the reference, never read
        self.difficulty_params = {
            "easy": {"device": "cpu", "bg_weight": 0.1, "planning_steps": 2, "num_simulations": 100,
                     "c_puct": 1.4, "exploration": 0.2},
            "medium": {"device": "cpu", "bg_weight": 0.2, "planning_steps": 3, "num_simulations": 200,
                       "c_puct": 1.6, "exploration": 0.05},
            "hard": {"device": "cpu", "bg_weight": 0.25, "planning_steps": 4, "num_simulations": 400,
                     "c_puct": 1.8, "exploration": 0.01},
        }
        self.params = self.difficulty_params.get(difficulty, self.difficulty_params["medium"])
        self.seed = random.getrandbits(64) if seed is None else int(seed)
        self.game_id = int(game_id)
        self.compute_priors = bool(compute_priors)
        self.games_played = 0
        self._last_decision_time = None
        self.last_search_stats = None
        self._used = False       # has searched in the current game
        self._last_count = -1    # move count of the last get_move board

    # a new game moves the AI's streams this far in game-id space, so the ids a
    # caller assigns to parallel games (0, 1, 2, ...) never meet a later game's
    GAME_ID_STRIDE = 1 << 32

    def new_game(self):
        """Start a new game: the next get_move draws from fresh streams.  The
        reference draws every game from the running global ``random``; here the
        streams are keyed by game id, so a reused AI moves to the next id (the
        first game keeps the constructor's ``game_id``)."""
        if self._used:
            self.game_id += self.GAME_ID_STRIDE
        self._used = False
        self._last_count = -1

    def _search_params(self, gather):
        return device.search_params(self.params.get("num_simulations", 200), self.params["c_puct"],
                                    self.params["exploration"], self.beta, self.seed, 100, self.planner_steps,
                                    gather)

    def get_move(self, board: GomokuBoard) -> Optional[Tuple[int, int]]:
        """ai_agent.py:109-136 (opening book, MCTS, exploration) on the GPU.
        A board with fewer stones than the last one this AI saw (a reset or a
        new board in a UI loop) starts a new game (``new_game``)."""
        n = board.get_move_count()
        if n < self._last_count:
            self.new_game()
        self._last_count = n
        self._used = True
        return self.get_moves([board], [self.game_id])[0]

    def get_moves(self, boards: List[GomokuBoard], game_ids: List[int]) -> List[Optional[Tuple[int, int]]]:
        """get_move for many boards in one batched search: board i draws from the
        streams of (self.seed, game_ids[i]), so the result equals get_move on each
        board with ``game_id = game_ids[i]``."""
        if self.search == "puct":
            return self._puct_moves(boards, game_ids)
        t0 = time.time()
        out = [None] * len(boards)
        # per board: the search's (predicts, main_draws, sim_draws); None if no search ran
        self.last_batch_stats = [None] * len(boards)
        groups = {}  # openings (< 6 plies) draw no simulation; the rest search
        for i, b in enumerate(boards):
            if b.get_valid_moves():
                groups.setdefault(b.get_move_count() >= 6, []).append(i)
        for needs_search, idx in sorted(groups.items()):
            gather = self.compute_priors and needs_search
            if needs_search:
                p = self._search_params(gather)
            else:
                p = device.search_params(self.params.get("num_simulations", 200), self.params["c_puct"],
                                         self.params["exploration"], self.beta, self.seed, 100, 0, False)
            cap = (p.num_simulations + 1) * len(idx) if gather else 0
            states = np.concatenate([boards[i].to_state() for i in idx])
            gids = [int(game_ids[i]) for i in idx]
            if needs_search and self.planner_steps and p.num_simulations > 0:
                mv, stats, _, leaves = device.plan_search(states, gids, p, self.bg_planner.planner_params(),
                                                          self.bg_planner.device_weights(), leaf_cap=cap)
            else:
                mv, stats, _, leaves = device.search(states, gids, p, leaf_cap=cap)
            if gather and leaves is not None and len(leaves):
                from gzero import boards as gb
                self.model.predict_batch(gb.words_to_cells(leaves[:, :8], leaves[:, 8:]))
            for k, i in enumerate(idx):
                m = int(mv[k])
                out[i] = None if m < 0 else (m // 15, m % 15)
                self.last_batch_stats[i] = (int(stats[k]["predicts"]), int(stats[k]["main_draws"]),
                                            int(stats[k]["sim_draws"]))
            self.last_search_stats = stats[-1]
        self._last_decision_time = time.time() - t0
        self.games_played += len(boards)
        return out

    def _puct_moves(self, boards, game_ids):
        """search="puct": the network-guided search (gz_puct_search) with the model's
        packed weights on every ply -- no opening book, no exploration move; beta and
        planner_steps are not used.  Sets last_search_visits and last_root_value."""
        t0 = time.time()
        out = [None] * len(boards)
        self.last_batch_stats = [None] * len(boards)
        if boards:
            w = self.model.device_weights()
            p = device.puct_params(self.params.get("num_simulations", 200), self.params["c_puct"], self.temp_plies,
                                   self.seed, w.precision, leaves_per_round=self.leaves_per_round,
                                   leaf_symmetry=self.leaf_symmetry)
            states = np.concatenate([b.to_state() for b in boards])
            mv, visits, q, _ = device.puct_search(states, [int(g) for g in game_ids], p, w)
            self.last_search_visits, self.last_root_value = visits, q
            for i, m in enumerate(mv):
                out[i] = None if int(m) < 0 else (int(m) // 15, int(m) % 15)
        self._last_decision_time = time.time() - t0
        self.games_played += len(boards)
        return out

    def evaluate_position(self, board: GomokuBoard) -> float:
        if board.game_over:
            if board.winner == self.player:
                return 1.0
            return -1.0 if board.winner is not None else 0.0
        _, value = self.model.predict(board.get_board_state())
        return value

    def _auto_save_model(self):
        try:
            return self.model.auto_save_model(suffix=f"_{self.difficulty}")
        except Exception as e:  # ai_agent.py:484-485 logs and continues
            self.logger.error(f"Failed to auto-save model: {e}")


class AIFactory:
    @staticmethod
    def create_ai(ai_type: str, player: int, difficulty: str = "medium", **kwargs):
        if ai_type == "alphazero":
            return AlphaZeroGomokuAI(player, difficulty, **kwargs)
        if ai_type == "bg_planner":
            return BGPlannerAI(player, difficulty, device=kwargs.get("device", "cpu"))
        raise ValueError(f"Unsupported ai_type: {ai_type}")

    @staticmethod
    def get_available_ai_types() -> List[str]:
        return ["alphazero", "bg_planner"]

    @staticmethod
    def get_available_difficulties() -> List[str]:
        return ["easy", "medium", "hard"]


def test_ai():
    """Module smoke check, as the reference's (ai_agent.py:626-660): one medium move on
    the empty board, its position evaluation and the auto-save; failures are printed,
    not raised (like the reference's)."""
    board = GomokuBoard()
    try:
        ai = AIFactory.create_ai("alphazero", board.BLACK, "medium")
        t0 = time.time()
        move = ai.get_move(board)
        print(f"move {move} in {time.time() - t0:.3f}s | evaluation {ai.evaluate_position(board):.3f}")
        ai._auto_save_model()
        print("AlphaZero AI smoke check passed")
    except Exception as e:  # noqa: BLE001 (reported, as the reference does)
        print(f"AlphaZero AI smoke check failed: {e}")


if __name__ == "__main__":
    test_ai()
