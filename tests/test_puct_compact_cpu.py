"""PUCT slot compaction without a GPU: the numpy restatement of the hole-filling plan
(tests/puct_compact_ref.py), the engine's argument checks and the library surface."""
import ctypes
import os

import numpy as np
import pytest

import puct_compact_ref as CR
from conftest import REPO
from gzero import _lib

NEW_ENTRY_POINTS = ("gz_selfplay_puct_run_active", "gz_selfplay_puct_rounds_active", "gz_selfplay_puct_layout",
                    "gz_selfplay_puct_compact")


def _masks():
    rng = np.random.default_rng(5)
    yield np.zeros(0, bool)
    for n in (1, 2, 7, 8, 64, 65, 1500):
        yield np.zeros(n, bool)               # none active
        yield np.ones(n, bool)                # all active
        yield np.arange(n) % 2 == 0           # alternating, an active slot first
        yield np.arange(n) % 2 == 1           # alternating, an idle slot first
        yield np.arange(n) < n // 2           # idle slots only at the tail
        yield np.arange(n) >= n // 2          # idle slots only in front
        for p in (0.1, 0.5, 0.9):
            yield rng.random(n) < p


def test_the_plan_fills_the_holes_from_the_tail():
    pairs = 0
    for active in _masks():
        n = len(active)
        a, holes, fillers, order = CR.plan(active)
        assert a == int(active.sum())
        assert len(holes) == len(fillers) and not set(holes) & set(fillers)
        assert (holes < a).all() and (fillers >= a).all()
        assert not active[holes].any() and active[fillers].all()
        assert list(holes) == sorted(holes) and list(fillers) == sorted(fillers)
        assert sorted(order) == list(range(n))  # a permutation
        after = np.zeros(n, bool)
        after[order] = active
        assert after[:a].all() and not after[a:].any()  # the active slots in front
        moved = np.flatnonzero(order != np.arange(n))
        assert set(moved) == set(holes) | set(fillers)  # the identity except at the pairs
        assert (order[order] == np.arange(n)).all()     # the pairs trade places
        a2, h2, f2, o2 = CR.plan(after)
        assert a2 == a and len(h2) == 0 and (o2 == np.arange(n)).all()  # a second compaction is the identity
        pairs += len(holes)
    assert pairs > 100


def test_new_entry_points_are_declared_and_check_their_arguments():
    L = _lib.load()
    hdr = open(os.path.join(REPO, "include", "gzero.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert hasattr(L, name) and name in _lib.SIGNATURES and f"int {name}(" in hdr, name
    assert hasattr(L, "gz_selfplay_puct_compact_workspace_bytes")
    assert "gz_selfplay_puct_compact_workspace_bytes" in _lib.SIGNATURES
    assert L.gz_selfplay_puct_compact_workspace_bytes(8) >= 4 + 2 * 8 * 4
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call below fails its argument checks
    p = _lib.PuctParams(16, 0, 1.6, 0, _lib.GZ_PV_F16X3, 0)
    pp = ctypes.byref(p)
    # n_active outside [1, n_slots]
    for entry in (L.gz_selfplay_puct_run_active, L.gz_selfplay_puct_rounds_active):
        for n_active in (0, -1, 9):
            assert entry(fake, 8, n_active, pp, fake, fake, 1, fake, 0, fake, fake, None) == -1
            assert b"n_active" in L.gz_last_error()
        assert entry(None, 8, 8, pp, None, None, 1, None, 0, None, None, None) == -1
    for n_active in (0, -1, 9):
        assert L.gz_selfplay_puct_compact(fake, 8, n_active, 16, 1, 0, fake, fake, fake, fake, None) == -1
        assert b"n_active" in L.gz_last_error()
    assert L.gz_selfplay_puct_compact(None, 8, 8, 16, 1, 0, None, None, None, None, None) == -1
    assert L.gz_selfplay_puct_compact(fake, 8, 8, 100000, 1, 0, fake, fake, fake, fake, None) == -1
    assert b"num_simulations" in L.gz_last_error()
    # tree reuse has no leaf batching, so a batched engine has no trees to move
    assert L.gz_selfplay_puct_compact(fake, 8, 8, 16, 4, 1, fake, fake, fake, fake, None) == -1
    assert b"leaves_per_round" in L.gz_last_error()
    assert L.gz_selfplay_puct_compact(fake, 8, 8, 16, 33, 0, fake, fake, fake, fake, None) == -1


def test_the_layout_places_pend_and_the_trees_by_the_capacity():
    L = _lib.load()
    al = lambda x: (x + 255) & ~255
    for n, S, K in ((1, 1, 0), (8, 16, 1), (8, 16, 4), (7, 200, 0), (4096, 200, 32)):
        out = (ctypes.c_size_t * 4)()
        assert L.gz_selfplay_puct_layout(n, S, K, out) == 0
        pend, block, tree0, stride = (int(x) for x in out)
        assert pend % 256 == 0 and block - pend == al(n * CR.PEND_SLOT_BYTES)
        assert tree0 == block + 256 and stride == al(128 + sum(CR.TREE_WIDTHS) * (S + 1))
        total = L.gz_selfplay_puct_batch_workspace_bytes(n, S, K) if K > 1 else L.gz_selfplay_puct_workspace_bytes(n, S)
        assert tree0 + n * stride < total
        # the PUCT block is what follows pend: the rest of the workspace is its size
        rest = L.gz_puct_batch_workspace_bytes(n, S, K) if K > 1 else L.gz_puct_workspace_bytes(n, S)
        assert block + rest == total
    out = (ctypes.c_size_t * 4)()
    assert L.gz_selfplay_puct_layout(0, 16, 0, out) == -1
    assert L.gz_selfplay_puct_layout(8, 16, 33, out) == -1
    assert L.gz_selfplay_puct_layout(8, 16, 0, None) == -1


def test_engine_argument_checks():
    from gzero.selfplay import SelfPlayEngine
    # (each raises before the library or a GPU is asked for)
    with pytest.raises(ValueError, match="compact_slots"):
        SelfPlayEngine(n_slots=8, compact_slots=True, game_id_end=8)  # needs search="puct"
    with pytest.raises(ValueError, match="compact_slots"):
        SelfPlayEngine(n_slots=8, search="puct", pv_weights=object(), compact_slots=True)  # needs a game_id_end
    import inspect
    import training
    assert inspect.signature(training.selfplay_puct_device).parameters["compact"].default is True
