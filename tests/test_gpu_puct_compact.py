"""Slot compaction of a PUCT engine on the GPU (csrc/gz_puct_compact.hip: gz_selfplay_puct_compact,
gz_selfplay_puct_run_active, gz_selfplay_puct_rounds_active): the games do not depend on
it, the move itself against the numpy restatement in tests/puct_compact_ref.py, its
edges, a workspace carved for its capacity and run for fewer slots, and the training
collection.  Every comparison is ==."""
import ctypes

import numpy as np
import pytest
import torch

import puct_compact_ref as CR
from gzero import _lib, device
from gzero.boards import RECORD_DTYPE
from gzero.device import ptr, stream
from gzero.selfplay import SelfPlayEngine
from test_gpu_puct import C_PUCT, _weights

pytestmark = pytest.mark.gpu

MODES = {"lockstep": {}, "leaves4": {"leaves_per_round": 4}, "reuse": {"tree_reuse": True},
         "reuse_noise": {"tree_reuse": True, "dirichlet_alpha": 0.3}}
SEED, TEMP = 21, 6


def _engine(mode, n_slots, S, game_id_end, compact_slots=True, **kw):
    return SelfPlayEngine(n_slots=n_slots, num_simulations=S, c_puct=C_PUCT, seed=SEED, pv_weights=_weights("f16x3"),
                          search="puct", temp_plies=TEMP, game_id_end=game_id_end, compact_slots=compact_slots,
                          **MODES[mode], **kw)


def _finished(eng):
    """(records, visit rows) of the games that ended in the last step, sorted by (id, ply)."""
    c = eng.counters()
    assert c["records_dropped"] == 0
    if not c["records"]:
        return np.zeros(0, RECORD_DTYPE), np.zeros((0, 225), np.uint16), int(c["games"])
    recs, vis = eng.records().copy(), eng.visits().copy()
    order = np.lexsort((recs["ply"], recs["game_id"]))
    return recs[order], vis[order], int(c["games"])


def _compact(eng):
    """compact() and the read of the count, as the training loop does; returns the count."""
    eng.n_active = int(eng.compact().item())
    return eng.n_active


# ---------------------------------------------------------------- 1. the same games
def _play_all(mode, n_slots, S, n_games, compacting):
    eng = _engine(mode, n_slots, S, n_games)
    recs, vis, done, steps, counts = [], [], 0, 0, []
    max_steps = (-(-n_games // n_slots)) * 200 + 8  # a step plays at least one move per live slot
    while done < n_games and steps < max_steps:
        eng.step()
        steps += 1
        r, v, g = _finished(eng)
        recs.append(r)
        vis.append(v)
        done += g
        if compacting:
            counts.append((done, _compact(eng)))
    assert done == n_games, (done, steps)
    recs, vis = np.concatenate(recs), np.concatenate(vis)
    order = np.lexsort((recs["ply"], recs["game_id"]))
    return recs[order], vis[order], counts, steps


@pytest.mark.parametrize("mode", list(MODES))
def test_the_same_games_with_and_without_compaction(mode):
    n_slots, S, n_games = 4, 8, 11  # slot 3 has the games 3 and 7, the others three each
    a_recs, a_vis, counts, a_steps = _play_all(mode, n_slots, S, n_games, True)
    b_recs, b_vis, _, b_steps = _play_all(mode, n_slots, S, n_games, False)
    assert sorted(set(int(g) for g in a_recs["game_id"])) == list(range(n_games))
    assert len(a_recs) == len(b_recs) and a_recs.tobytes() == b_recs.tobytes()
    assert a_vis.dtype == b_vis.dtype and a_vis.tobytes() == b_vis.tobytes()
    assert (a_vis.sum(axis=1) == S).all()
    # fewer slots ran while games were still being played, and in the end none
    assert any(n < n_slots for done, n in counts if done < n_games), counts
    assert counts[-1] == (n_games, 0) and all(x[1] >= y[1] for x, y in zip(counts, counts[1:])), counts
    ran = [n for _, n in counts]
    print(f"{mode}: {len(a_recs)} plies, {a_steps} steps compacting / {b_steps} not; steps that left k slots active: "
          f"{ {k: ran.count(k) for k in range(n_slots, -1, -1)} }")


# ---------------------------------------------------------------- 2. and 3. the move itself
def _layout(eng):
    out = (ctypes.c_size_t * 4)()
    _lib.check(eng.lib.gz_selfplay_puct_layout(eng.n_slots, eng.puct.num_simulations, eng.leaves_per_round, out),
               "gz_selfplay_puct_layout")
    return [int(x) for x in out]


def _snapshot(eng):
    """Host copies: slots uint8 [n, slot_bytes], the workspace uint8 [bytes], the parsed tree exports."""
    n, S = eng.n_slots, eng.puct.num_simulations
    slots = eng.d_slots.cpu().numpy().reshape(n, -1).copy()
    ws = eng.d_puct_ws.cpu().numpy().copy()
    trees = device._puct_trees(eng.lib, eng.d_puct_ws[_layout(eng)[1]:], n, S)
    return slots, ws, trees


def _check_compaction(eng, n_active=None):
    """Compact the first n_active slots and compare everything with the numpy restatement;
    returns (a, holes, fillers)."""
    n, S = eng.n_slots, eng.puct.num_simulations
    if n_active is not None:
        eng.n_active = n_active
    n_act = eng.n_active
    lay = _layout(eng)
    rounds0 = lay[2] + n * lay[3]  # the round buffers (scratch) begin here
    slots, ws, trees = _snapshot(eng)
    a, holes, fillers, order = CR.plan(CR.active_mask(slots[:n_act]))
    eng.d_order.fill_(-7)
    d_a = eng.compact()
    assert int(d_a.item()) == a
    got = eng.d_order.cpu().numpy()
    assert list(got[:n_act]) == list(order) and (got[n_act:] == -7).all()
    slots2, ws2, trees2 = _snapshot(eng)
    # the slot buffer: the snapshot permuted (new[order[s]] = old[s]; slots past n_active stay)
    perm = np.arange(n)
    perm[:n_act] = order
    assert np.array_equal(slots2[perm], slots)
    assert np.array_equal(slots2, CR.expected_slots(slots, n_act))
    # every filler's tree (the export cuts each array at n_nodes) and pending rows at its new index
    n_moves = CR.slot_field(slots, CR.SLOT_N_MOVES, np.int32)
    for h, f in zip(holes, fillers):
        if eng.tree_reuse:
            assert trees2[h].keys() == trees[f].keys()
            for key in trees[f]:
                assert np.array_equal(trees2[h][key], trees[f][key]), (h, f, key)
        nb = int(n_moves[f]) * 450
        src, dst = lay[0] + f * CR.PEND_SLOT_BYTES, lay[0] + h * CR.PEND_SLOT_BYTES
        assert np.array_equal(ws2[dst:dst + nb], ws[src:src + nb]), (h, f)
    # the active slots that stayed: their trees as they were
    for s in np.flatnonzero(CR.active_mask(slots[:n_act])):
        if s not in fillers:
            for key in trees[s]:
                assert np.array_equal(trees2[s][key], trees[s][key]), (s, key)
    # the whole workspace below the round buffers: the moved ranges moved, every other byte as it was
    want = CR.expected_workspace(ws, slots, n_act, lay, S, eng.tree_reuse)
    assert np.array_equal(ws2[:rounds0], want[:rounds0])
    if len(holes) == 0:
        assert np.array_equal(ws2[:rounds0], ws[:rounds0])
    return a, holes, fillers


def _set_ends(eng, ends):
    """game_id_end of every slot (SlotHeader, csrc/gz_search.h), straight into the slot buffer."""
    view = eng.d_slots.view(torch.int64).view(eng.n_slots, -1)
    view[:, CR.SLOT_GAME_ID_END // 8] = torch.as_tensor(ends, dtype=torch.int64, device="cuda")


def _set_active(eng, active):
    gid = CR.slot_field(eng.d_slots.cpu().numpy().reshape(eng.n_slots, -1), CR.SLOT_GAME_ID, np.int64)
    _set_ends(eng, np.where(active, gid + 1, gid))


def test_the_move_itself_with_tree_reuse():
    n, S = 8, 16
    eng = _engine("reuse", n, S, 10 ** 9, rounds_per_step=S + 1)
    done, steps = 0, 0
    while done == 0 and steps < 220:  # until a slot has finished its first game
        eng.step()
        steps += 1
        done += int(eng.counters()["games"])
    assert done > 0, steps
    # exactly the slots that finished (they hold the games n, n + 1, ...) go idle
    _lib.check(eng.lib.gz_selfplay_set_game_end(ptr(eng.d_slots), n, n, stream()), "gz_selfplay_set_game_end")

    def holes_now():
        act = CR.active_mask(eng.d_slots.cpu().numpy().reshape(n, -1))
        return len(CR.plan(act)[1]), int(act.sum())
    while holes_now()[0] == 0 and holes_now()[1] > 0 and steps < 440:
        eng.step()
        steps += 1
    n_holes, n_act = holes_now()
    assert n_holes > 0, f"no idle slot below the active count after {steps} steps ({n_act} active)"
    a, holes, fillers = _check_compaction(eng)
    assert a == n_act and len(holes) == n_holes
    # the fillers brought live trees and rows
    slots = eng.d_slots.cpu().numpy().reshape(n, -1)
    assert (CR.slot_field(slots, CR.SLOT_N_MOVES, np.int32)[holes] > 0).all()
    # and the engine plays on with the a slots
    eng.n_active = a
    eng.step()
    assert eng.counters()["records_dropped"] == 0


@pytest.fixture(scope="module", params=["reuse", "lockstep"])
def warm_engine(request):
    """8 slots a few plies into their first games: live trees (reuse) and pending rows."""
    n, S = 8, 16
    kw = {"rounds_per_step": 5 * (S + 1)} if request.param == "reuse" else {"plies_per_step": 5}
    eng = _engine(request.param, n, S, 10 ** 9, **kw)
    eng.step()
    slots = eng.d_slots.cpu().numpy().reshape(n, -1)
    assert (CR.slot_field(slots, CR.SLOT_N_MOVES, np.int32) >= 4).all()
    return eng


def test_edges(warm_engine):
    eng = warm_engine
    n = eng.n_slots
    every = np.ones(n, bool)
    cases = [("no idle slot", every, n, 0), ("all idle", ~every, n, 0),
             ("idle slots only at the tail", np.arange(n) < 5, n, 0),
             ("alternating", np.arange(n) % 2 == 1, n, 2),
             ("idle slots in front", np.arange(n) >= 3, n, 3),
             ("one slot, active", every, 1, 0), ("one slot, idle", ~every, 1, 0),
             ("the first five of a mixed buffer", np.array([0, 1, 0, 1, 1, 0, 1, 1], bool), 5, 2)]
    for name, active, n_active, pairs in cases:
        _set_active(eng, active)  # (by position: the slots were permuted by the cases before)
        a, holes, fillers = _check_compaction(eng, n_active)
        assert len(holes) == pairs and a == int(active[:n_active].sum()), name
        # a second compaction right after the first is the identity
        a2, holes2, _ = _check_compaction(eng, n_active)
        assert a2 == a and len(holes2) == 0, name
    _set_active(eng, every)
    eng.n_active = n


def test_bad_arguments_launch_nothing(warm_engine):
    eng = warm_engine
    n, S = eng.n_slots, eng.puct.num_simulations
    _set_active(eng, np.arange(n) % 2 == 1)  # a compaction would move something
    before = _snapshot(eng)
    eng.d_order.fill_(-7)
    eng.d_n_active.fill_(-7)

    def call(n_active, K, move_trees):
        return eng.lib.gz_selfplay_puct_compact(ptr(eng.d_slots), n, n_active, S, K, move_trees, ptr(eng.d_puct_ws),
                                                ptr(eng.d_order), ptr(eng.d_n_active), ptr(eng.d_compact_ws), stream())
    for n_active in (0, -3, n + 1):
        assert call(n_active, 1, 0) == -1 and b"n_active" in eng.lib.gz_last_error()
    assert call(n, 4, 1) == -1 and b"leaves_per_round" in eng.lib.gz_last_error()
    p = ctypes.byref(eng.puct)
    for entry in (eng.lib.gz_selfplay_puct_run_active, eng.lib.gz_selfplay_puct_rounds_active):
        for n_active in (0, n + 1):
            assert entry(ptr(eng.d_slots), n, n_active, p, ptr(eng.pv_weights.tensor), ptr(eng.d_puct_ws), 1,
                         ptr(eng.d_records), eng.record_cap, ptr(eng.d_visits), ptr(eng.d_counters), stream()) == -1
    after = _snapshot(eng)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert (eng.d_order.cpu().numpy() == -7).all() and int(eng.d_n_active.item()) == -7
    _set_active(eng, np.ones(n, bool))


def test_engine_without_compact_slots_still_refuses():
    eng = _engine("lockstep", 4, 8, 4, compact_slots=False)
    with pytest.raises(ValueError):
        eng.compact()
    with pytest.raises(ValueError):
        SelfPlayEngine(n_slots=4, num_simulations=8, pv_weights=_weights("f16x3"), search="puct", compact_slots=True)


# ---------------------------------------------------------------- 4. capacity against active count
def test_fewer_active_slots_play_the_same_moves():
    """A lock-step engine of 8 slots compacted after every ply against its twin that
    never is: after every single step the surviving games stand at the same boards and
    the games that ended left the same records and visit rows -- the pending rows and
    the trees are found where the capacity put them, whatever the active count."""
    n, S, n_games = 8, 8, 12
    a_eng, b_eng = _engine("lockstep", n, S, n_games), _engine("lockstep", n, S, n_games, compact_slots=False)
    done, steps, shrunk = 0, 0, 0
    while done < n_games and steps < 2 * 200 + 8:
        a_eng.step()
        b_eng.step()
        steps += 1
        ar, av, ag = _finished(a_eng)
        br, bv, bg = _finished(b_eng)
        assert ag == bg and ar.tobytes() == br.tobytes() and av.tobytes() == bv.tobytes(), steps
        done += ag
        n_act = _compact(a_eng)
        shrunk += 0 < n_act < n
        (ast, agid), (bst, bgid) = a_eng.boards(), b_eng.boards()
        live = {int(g): s for s, g in enumerate(bgid) if g < n_games}
        assert sorted(int(g) for g in agid[:n_act]) == sorted(live), steps
        for s in range(n_act):
            assert ast[s].tobytes() == bst[live[int(agid[s])]].tobytes(), (steps, s)
    assert done == n_games and a_eng.n_active == 0
    assert shrunk > 10, shrunk  # many plies were played by fewer slots than the capacity


# ---------------------------------------------------------------- 5. training
@pytest.mark.parametrize("tree_reuse", [False, True])
def test_selfplay_puct_device_compacts_to_the_same_rows(tree_reuse):
    import training
    from gzero.train import DeviceTrainer
    from test_gpu_puct_train import _model
    model = _model()
    DeviceTrainer(model)
    out = {}
    for compact in (True, False):
        d, d_vis, n, st = training.selfplay_puct_device(6, num_simulations=8, seed=11, game_id_base=12, model=model,
                                                        temp_plies=TEMP, plies_per_step=2, tree_reuse=tree_reuse,
                                                        compact=compact)
        out[compact] = (d.cpu().numpy().tobytes(), d_vis.cpu().numpy().tobytes(), n, st)
    assert out[True][2] == out[False][2] > 0
    assert out[True][0] == out[False][0] and out[True][1] == out[False][1]
    recs = np.frombuffer(out[True][0], RECORD_DTYPE)
    assert sorted(set(int(g) for g in recs["game_id"])) == list(range(12, 18))
    assert out[True][3]["games"] == out[False][3]["games"] == 6
    assert out[True][3]["steps"] <= out[False][3]["steps"]
    assert out[True][3]["moves_played"] <= out[False][3]["moves_played"]
    print(f"tree_reuse={tree_reuse}: {out[True][2]} rows; steps {out[True][3]['steps']} / {out[False][3]['steps']}, "
          f"moves played {out[True][3]['moves_played']} / {out[False][3]['moves_played']} (compact / not)")
