"""The PUCT search mode without a GPU: the library surface (entry points, argument
checks, Python-side mode checks) and the plain-Python reference on a tactical
position whose numbers were worked out by hand from the semantics."""
import ctypes

import pytest

import puct_ref as R
from gzero import _lib


# ---------------------------------------------------------------- (a) library surface
def test_library_has_puct_entry_points():
    L = _lib.load()
    for name in ("gz_puct_workspace_bytes", "gz_puct_begin", "gz_puct_select", "gz_puct_backup", "gz_puct_finish",
                 "gz_puct_search", "gz_puct_tree_bytes", "gz_puct_trees", "gz_selfplay_puct_workspace_bytes",
                 "gz_selfplay_puct_run"):
        assert hasattr(L, name) and name in _lib.SIGNATURES, name
    assert ctypes.sizeof(_lib.PuctParams) == 32


def test_puct_search_rejects_bad_arguments():
    L = _lib.load()
    p = _lib.PuctParams(100000, 0, 1.6, 0, _lib.GZ_PV_F16X3, 0)
    args = (None, None, 1, ctypes.byref(p), None, None, None, None, None, None)
    assert L.gz_puct_search(*args) == -1 and b"num_simulations" in L.gz_last_error()
    p.num_simulations = 0
    assert L.gz_puct_search(*args) == -1
    p.num_simulations = 16
    p.precision = 7
    assert L.gz_puct_search(*args) == -1 and b"precision" in L.gz_last_error()
    p.precision = _lib.GZ_PV_FP32
    assert L.gz_puct_search(*args) == -1  # NULL pointers
    assert L.gz_puct_search(None, None, 1, None, None, None, None, None, None, None) == -1
    assert L.gz_puct_select(None, 1, 100000, None, None, None) == -1
    assert L.gz_selfplay_puct_run(None, 1, ctypes.byref(p), None, None, 1, None, 0, None, None, None) == -1


def test_puct_sizes():
    L = _lib.load()
    M = 201
    # W, prior row, visits, value, board, parent, move, term per node
    assert L.gz_puct_tree_bytes(200) >= M * (8 + 1800 + 4 + 4 + 64 + 2 + 1 + 1)
    assert L.gz_puct_tree_bytes(200) > 0
    # the tree plus the child table: about 2.3 KB per node
    per_game = (L.gz_puct_workspace_bytes(1024, 200) - L.gz_puct_workspace_bytes(1024, 100)) / 1024 / 100
    assert 2300 <= per_game <= 2400
    assert L.gz_selfplay_puct_workspace_bytes(8, 16) > L.gz_puct_workspace_bytes(8, 16) + 8 * 200 * 225 * 2


def test_python_mode_checks():
    from ai_agent import AIFactory, AlphaZeroGomokuAI
    from gzero.selfplay import SelfPlayEngine
    with pytest.raises(ValueError):
        AlphaZeroGomokuAI(1, search="bogus")
    with pytest.raises(ValueError):
        AIFactory.create_ai("alphazero", 1, search="bogus")
    with pytest.raises(ValueError):
        SelfPlayEngine(n_slots=8, search="bogus")
    with pytest.raises(ValueError):
        SelfPlayEngine(n_slots=8, search="puct")  # no pv_weights
    with pytest.raises(ValueError):
        SelfPlayEngine(n_slots=8, search="puct", pv_weights=object(), planner_steps=2)
    ai = AlphaZeroGomokuAI(1, search="puct", seed=1)
    assert ai.search == "puct" and ai.last_search_visits is None and ai.last_root_value is None


# ---------------------------------------------------------------- (b) the reference
def test_reference_finds_the_five_at_120_simulations():
    cells, player, n_moves = R.tactical_position()
    t = R.search(cells, player, n_moves, 120, 1.6, R.uniform_eval)
    v = t.root_visits()
    assert len(t.parent) == 107
    assert t.visits[0] == 121
    assert v[107] == 15 and v[112] == 0
    assert sorted(x for c, x in enumerate(v) if x and c != 107) == [1] * 105
    assert sum(v) == 120
    j = t.child[0][107]
    assert t.term[j] == 1 and t.W[j] == 15.0 and t.child[j] == {}
    assert R.choose_move(t, 0, 0, 0) == (107, 0)
    # 106 value-0 evaluations and 15 wins for the side to move
    assert R.root_q(t) == 15.0 / 121.0


def test_reference_misses_it_at_60_simulations():
    cells, player, n_moves = R.tactical_position()
    t = R.search(cells, player, n_moves, 60, 1.6, R.uniform_eval)
    v = t.root_visits()
    assert v[107] == 0 and len(t.parent) == 61
    assert R.choose_move(t, 0, 0, 0) == (1, 0)


def test_reference_sampling_is_the_rng_pick():
    from gzero import rng
    cells, player, n_moves = R.tactical_position()
    t = R.search(cells, player, n_moves, 120, 1.6, R.uniform_eval)
    v = t.root_visits()
    seen = set()
    for gid in range(8):
        mv, draws = R.choose_move(t, 9, 5, gid)
        pick = (rng.draw(rng.stream_key(5, gid, 8, 0), 0) * 120) >> 64
        assert draws == 1 and sum(v[:mv]) <= pick < sum(v[:mv + 1])
        seen.add(mv)
    assert len(seen) > 1
