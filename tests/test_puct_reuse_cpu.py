"""PUCT tree reuse without a GPU: the plain-Python restatement (tests/puct_reuse_ref.py)
against tests/puct_ref.py, the properties the kernels rely on, and the library surface."""
import ctypes
import os

import numpy as np
import pytest

import puct_ref as R
import puct_reuse_ref as RR
from conftest import REPO
from gzero import _lib
from test_gpu_puct import C_PUCT, _thinned, make_synth

NEW_ENTRY_POINTS = ("gz_puct_reroot", "gz_selfplay_puct_rounds", "gz_selfplay_puct_reset")


def _same_tree(a, b):
    for f in ("parent", "move", "term", "visits", "W", "child", "prior", "value", "cells", "player", "count"):
        assert getattr(a, f) == getattr(b, f), f


@pytest.mark.parametrize("S", [1, 2, 40])
def test_fresh_and_simulate_restate_the_search(S):
    evalf = make_synth()
    for cells, n_moves in (([0] * 225, 0), ([int(x) for x in _thinned(41, 1)], 41)):
        player = 1 + n_moves % 2
        t = RR.fresh(cells, player, n_moves, evalf)
        for _ in range(S):
            RR.simulate(t, C_PUCT, evalf)
        _same_tree(t, R.search(cells, player, n_moves, S, C_PUCT, evalf))  # floats with ==: bit for bit
        assert t.visits[0] == S + 1


def test_reroot_keeps_creation_order_and_remaps_children():
    evalf = make_synth()
    t = R.search([0] * 225, 1, 0, 40, C_PUCT, evalf)
    j = max(t.child[0].values(), key=lambda k: t.visits[k])
    nt = RR.reroot(t, j)
    # the kept nodes are j and its descendants, in their old order
    kept = [k for k in range(len(t.parent)) if k == j or _is_below(t, k, j)]
    assert len(nt.parent) == len(kept) >= 3 and kept == sorted(kept) and kept[0] == j
    assert nt.parent[0] == -1 and nt.move[0] == 255
    for new, old in enumerate(kept):
        assert nt.cells[new] == t.cells[old] and nt.visits[new] == t.visits[old] and nt.W[new] == t.W[old]
        assert nt.prior[new] is t.prior[old] and nt.value[new] == t.value[old] and nt.term[new] == t.term[old]
        assert nt.child[new] == {c: kept.index(x) for c, x in t.child[old].items()}
        if new:
            assert nt.parent[new] == kept.index(t.parent[old]) < new and nt.move[new] == t.move[old]
            assert nt.child[nt.parent[new]][nt.move[new]] == new
    assert nt.count[0] == 1 and nt.player[0] == 2
    # the subtree of a leaf is that leaf
    leaf = len(t.parent) - 1
    assert len(RR.reroot(t, leaf).parent) == 1


def _is_below(t, k, j):
    while k >= 0:
        if k == j:
            return True
        k = t.parent[k]
    return False


def test_properties_on_whole_games():
    S, temp, seed = 16, 6, 21
    evalf = make_synth()
    for gid in (0, 1):
        seen = []

        def on_ply(ply, before, after, seen=seen):
            assert len(before.parent) <= S + 1 and before.visits[0] == S + 1
            if after is not None:
                j = before.child[0][moves_so_far(before, after)]
                assert len(after.parent) <= before.visits[j]  # kept nodes <= visits[child]
                assert after.visits[0] == before.visits[j] <= S
            seen.append((before.visits[0], None if after is None else after.visits[0]))

        def moves_so_far(before, after):
            (c,) = [c for c in range(225) if before.cells[0][c] != after.cells[0][c]]
            return c

        moves, rows, z, rounds = RR.play_game(seed, gid, S, C_PUCT, temp, evalf, on_ply=on_ply)
        cells = [0] * 225
        for k, m in enumerate(moves):
            assert cells[m] == 0 and sum(rows[k]) == S and rows[k][m] > 0
            assert not any(v for v, x in zip(rows[k], cells) if x)
            if k >= temp:
                assert m == int(np.argmax(rows[k]))
            cells[m] = 1 + k % 2
        # a root that inherits v visits plays after S + 1 - v rounds, at least one
        assert rounds[0] == S + 1
        for k in range(1, len(moves)):
            assert rounds[k] == S + 1 - seen[k - 1][1] >= 1
        assert sum(rounds) < (S + 1) * len(moves)
        assert len(set(z)) <= 2 and len(z) == len(moves)
        # without reuse the same evaluator plays S + 1 rounds per move
        m2, r2, _, rounds2 = RR.play_game(seed, gid, S, C_PUCT, temp, evalf, reuse=False, max_plies=4)
        assert rounds2 == [S + 1] * 4 and m2[0] == moves[0] and r2[0] == rows[0]


def test_new_entry_points_are_declared_and_check_their_arguments():
    L = _lib.load()
    hdr = open(os.path.join(REPO, "include", "gzero.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert hasattr(L, name) and name in _lib.SIGNATURES and f"int {name}(" in hdr, name
    p = _lib.PuctParams(16, 0, 1.6, 0, _lib.GZ_PV_F16X3, 0)
    assert L.gz_puct_reroot(None, 1, 16, None, None, None, None, None) == -1
    assert L.gz_puct_reroot(None, 1, 100000, None, None, None, None, None) == -1
    assert b"num_simulations" in L.gz_last_error()
    assert L.gz_puct_reroot(None, 0, 16, None, None, None, None, None) == 0
    assert L.gz_selfplay_puct_reset(None, 8, 16, None) == -1
    assert L.gz_selfplay_puct_rounds(None, 8, ctypes.byref(p), None, None, 1, None, 0, None, None, None) == -1
    p.precision = 7
    assert L.gz_selfplay_puct_rounds(None, 8, ctypes.byref(p), None, None, 1, None, 0, None, None, None) == -1
    assert b"precision" in L.gz_last_error()
    # the trees of a reuse engine fit the workspace of the lock-step one: same size call
    assert L.gz_selfplay_puct_workspace_bytes(8, 16) > L.gz_puct_workspace_bytes(8, 16)


def test_python_mode_checks():
    from gzero.selfplay import SelfPlayEngine
    import training
    with pytest.raises(ValueError):
        SelfPlayEngine(n_slots=8, tree_reuse=True)  # needs search="puct"
    with pytest.raises(ValueError):
        training.run_iteration(None, None, 0, tree_reuse=True)


def test_the_step_api_scenario_reuses_deep_and_shallow():
    """The inputs of test_gpu_puct_reuse's step-API test: some re-root keeps >= 8 nodes
    over >= 3 depths and some keeps exactly one."""
    from test_gpu_puct_reuse import STEP_GIDS, STEP_PLIES, STEP_SEED, STEP_SIMS, STEP_TEMP
    evalf = make_synth()
    kept = {}
    for S in STEP_SIMS:
        for gid in STEP_GIDS:
            def on_ply(ply, before, after, S=S):
                if after is not None:
                    depths = {RR.depth_of(after, k) for k in range(len(after.parent))}
                    kept.setdefault(S, []).append((len(after.parent), len(depths)))
            RR.play_game(STEP_SEED, gid, S, C_PUCT, STEP_TEMP, evalf, max_plies=STEP_PLIES, on_ply=on_ply)
    assert any(n >= 8 and d >= 3 for n, d in kept[64])
    assert any(n == 1 for n, d in kept[1]) and any(n == 1 for S in STEP_SIMS for n, d in kept[S])
