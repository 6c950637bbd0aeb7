"""The PUCT arena on the GPU (csrc/gz_puct_match.hip: gz_puct_match_run, gz_puct_match_results;
gzero/arena.py) against the self-play engine where both sides are one network, and against
the plain-Python driver of tests/puct_match_ref.py where they are two.  Every comparison
is ==."""
import ctypes

import numpy as np
import pytest
import torch

import puct_match_ref as MR
from gzero import _lib, arena, device, weights
from gzero.boards import RECORD_DTYPE, words_to_cells
from gzero.device import ptr, stream
from gzero.selfplay import SelfPlayEngine

pytestmark = pytest.mark.gpu

C_PUCT = 1.6
SEED, TEMP = 21, 4
_W, _DRIVE, _MODELS = {}, {}, {}


def _weights(seed, precision):
    if (seed, precision) not in _W:
        _W[seed, precision] = device.PVWeights(weights.pack_pv_weights(weights.init_state_dict(seed)), precision)
    return _W[seed, precision]


def _sides():
    """A: init_state_dict(0) in f16x3; B: init_state_dict(1) in f16."""
    return [_weights(0, "f16x3"), _weights(1, "f16")]


def _p(S, alpha=None):
    return {"num_simulations": S, "c_puct": C_PUCT, "temp_plies": TEMP, "seed": SEED, "dirichlet_alpha": alpha}


def _drive(ids, S, alpha, parity, max_plies=200):
    """The reference games, computed once per case and shared."""
    key = (tuple(ids), S, alpha, parity, max_plies)
    if key not in _DRIVE:
        _DRIVE[key] = MR.drive(ids, _sides(), _p(S, alpha), parity, max_plies)
    return _DRIVE[key]


def _match(sides, games, S, alpha=None, parity=0, base=0, stride=1, compact=True):
    return arena.PuctMatch(sides[0], sides[1], games, num_simulations=S, c_puct=C_PUCT, temp_plies=TEMP, seed=SEED,
                           dirichlet_alpha=alpha, game_id_base=base, a_black_parity=parity, game_id_stride=stride,
                           compact=compact)


def _games(recs, vis):
    """{id: (moves, visit rows, z per ply)} from records sorted by (id, ply)."""
    out = {}
    for gid in np.unique(recs["game_id"]):
        sel = recs["game_id"] == gid
        r = recs[sel]
        assert list(r["ply"]) == list(range(len(r))) and list(r["player"]) == [1 + k % 2 for k in range(len(r))]
        out[int(gid)] = ([int(x) for x in r["move"]], vis[sel].astype(np.int32), [int(x) for x in r["z"]])
    return out


def _assert_equals_drive(m, ref, S):
    recs, vis = m.records()
    got = _games(recs, vis)
    assert sorted(got) == sorted(ref)
    for gid, (moves, rows, z) in got.items():
        o = ref[gid]
        assert o["over"], gid
        assert moves == o["moves"], gid
        assert np.array_equal(rows, np.array(o["visits"], np.int32)), gid
        assert z == o["z"], gid
        assert (rows.sum(axis=1) == S).all()


# ---------------------------------------------------------------- 1. one network on both sides
@pytest.mark.parametrize("n", [5, 70])
def test_same_network_equals_selfplay(n):
    """Both sides the same blob and precision: records, visit rows and counters of every
    step are the bytes of the lock-step self-play engine (records and rows compared in (id,
    ply) order: games that end in one step take their places by an atomic).  70 slots
    cross a wavefront in the plan's scan."""
    S = 6
    w = _weights(0, "f16x3")
    m = _match([w, w], n, S, compact=False)
    eng = SelfPlayEngine(n_slots=n, num_simulations=S, c_puct=C_PUCT, seed=SEED, pv_weights=w, search="puct",
                         temp_plies=TEMP, game_id_end=n)
    steps = plies = 0
    while not m.finished():
        assert steps < 200
        m.step()
        eng.step()
        steps += 1
        assert m.d_counters.cpu().numpy().tobytes() == eng.d_counters.cpu().numpy().tobytes(), steps
        a, av = m.step_records()
        b, bv = eng.records(), eng.visits()
        assert len(a) == len(b), steps
        oa, ob = np.lexsort((a["ply"], a["game_id"])), np.lexsort((b["ply"], b["game_id"]))
        assert a[oa].tobytes() == b[ob].tobytes() and av[oa].tobytes() == bv[ob].tobytes(), steps
        plies += len(a)
    assert m.games_done == n and plies > 9 * n
    (ms, mg), (es, eg) = m.boards(), eng.boards()
    assert ms.tobytes() == es.tobytes() and list(mg) == list(eg)
    t = m.tally()
    assert t["games"] == n and t["plies"] == plies


# ---------------------------------------------------------------- 2. two networks
def test_the_reference_can_see_a_wrong_route():
    """From the reference alone: with the sides swapped (parity 1 is exactly that) at least
    one game is played differently, so a leaf sent to the wrong network would show."""
    ids = list(range(10, 16))
    a, b = _drive(ids, 8, None, 0), _drive(ids, 8, None, 1)
    assert any(a[g]["moves"] != b[g]["moves"] for g in ids)


@pytest.mark.parametrize("parity", [0, 1])
@pytest.mark.parametrize("alpha", [None, 0.3])
def test_two_networks_mixed_precisions(alpha, parity):
    S, ids = 8, list(range(10, 16))
    ref = _drive(ids, S, alpha, parity)
    m = _match(_sides(), 6, S, alpha=alpha, parity=parity, base=10)
    m.run()
    _assert_equals_drive(m, ref, S)
    t, res = m.tally(), m.results()
    for i, g in enumerate(ids):
        w = ref[g]["winner"]
        want = 0 if w == 0 else (1 if MR.side_of(g, w, parity) == 0 else -1)
        assert int(res[i]) == want, g
    assert t["games"] == 6 and t["plies"] == sum(len(ref[g]["moves"]) for g in ids)


# ---------------------------------------------------------------- 3. one side has no rows
def test_one_sided_plies():
    """All game ids even (slot s plays game 10 + 2 s), so every ply is moved by one side
    only and the other side's count is 0 in every round."""
    S, ids = 8, [10, 12, 14]
    assert all(len({MR.side_of(g, pl, 0) for g in ids}) == 1 for pl in (1, 2))
    ref = _drive(ids, S, None, 0)
    m = _match(_sides(), 3, S, base=10, stride=2)
    m.run()
    _assert_equals_drive(m, ref, S)
    assert [int(x) for x in m.results()] == [
        0 if ref[g]["winner"] == 0 else (1 if MR.side_of(g, ref[g]["winner"], 0) == 0 else -1) for g in ids]


# ---------------------------------------------------------------- 4. the plan's scan
def test_scan_edges():
    """130 slots (two full wavefronts and a remainder), the sides interleaved by id: the
    boards after each of three plies."""
    n, S = 130, 2
    ref = _drive(list(range(n)), S, None, 0, max_plies=3)
    m = _match(_sides(), n, S, compact=False)
    for k in range(3):
        m.step()
        st, gids = m.boards()
        assert list(gids) == list(range(n))
        cells = words_to_cells(st["black"], st["white"])
        for g in range(n):
            assert tuple(int(x) for x in cells[g]) == ref[g]["after"][k], (k, g)
        assert (st["n_moves"] == k + 1).all()


# ---------------------------------------------------------------- 5. compaction
def test_compaction_changes_nothing():
    S, n = 6, 12
    a = _match(_sides(), n, S, compact=True)
    moved = 0
    while not a.finished():
        before = a.n_active
        a.step()
        order = a.d_order.cpu().numpy()[:before]
        moved += int((order != np.arange(before)).any())
    assert a.n_active == 0 and moved > 0  # a compaction that moves no slot would show nothing
    b = _match(_sides(), n, S, compact=False)
    b.run()
    (ar, av), (br, bv) = a.records(), b.records()
    assert sorted(set(int(g) for g in ar["game_id"])) == list(range(n))
    assert ar.tobytes() == br.tobytes() and av.tobytes() == bv.tobytes()
    assert a.tally() == b.tally()


# ---------------------------------------------------------------- 6. results
def test_results():
    S, n, base = 6, 8, 10
    m = _match(_sides(), n, S, parity=1, base=base)
    m.run()
    recs, _ = m.records()
    want, res = MR.tally(recs, 1)
    t = m.tally()  # fed step by step
    assert t == want
    assert t["games"] == t["a_wins"] + t["b_wins"] + t["draws"] == n
    assert t["a_wins_black"] + t["a_wins_white"] == t["a_wins"] and t["b_wins_black"] + t["b_wins_white"] == t["b_wins"]
    assert [int(x) for x in m.results()] == [res[base + i] for i in range(n)]
    # ids outside [12, 15) are tallied and not written; the bytes around d_result stay
    d_recs = device.to_dev(recs)
    d_tally = torch.zeros(9, dtype=torch.int64, device="cuda")
    buf = torch.full((8 + 3 + 8,), 0x55, dtype=torch.int8, device="cuda")
    _lib.check(m.lib.gz_puct_match_results(ptr(d_recs), len(recs), 1, 12, 3, ptr(d_tally),
                                           ctypes.c_void_p(buf.data_ptr() + 8), stream()), "gz_puct_match_results")
    got = buf.cpu().numpy()
    assert (got[:8] == 0x55).all() and (got[11:] == 0x55).all()
    assert [int(x) for x in got[8:11]] == [res[12], res[13], res[14]]
    assert {k: int(v) for k, v in zip(MR.TALLY_FIELDS, d_tally.cpu().numpy())} == want
    # games not in the records leave their entries alone
    buf.fill_(0x55)
    some = recs[recs["game_id"] != 13]
    _lib.check(m.lib.gz_puct_match_results(ptr(device.to_dev(some)), len(some), 1, 12, 3, ptr(d_tally),
                                           ctypes.c_void_p(buf.data_ptr() + 8), stream()), "gz_puct_match_results")
    assert [int(x) for x in buf.cpu().numpy()[8:11]] == [res[12], 0x55, res[14]]


# ---------------------------------------------------------------- 7. the Python layer
def _model(seed):
    if seed not in _MODELS:
        from neural_network import GomokuModel
        model = GomokuModel(device="cpu")
        model.model.load_state_dict(weights.init_state_dict(seed=seed))
        _MODELS[seed] = model
    return _MODELS[seed]


def test_python_layer():
    import training
    S, ids = 8, list(range(10, 16))
    kw = dict(games=6, num_simulations=S, c_puct=C_PUCT, temp_plies=TEMP, seed=SEED, precision_a="f16x3",
              precision_b="f16", game_id_base=10)
    a, b = _model(0), _model(1)
    one = arena.play_match(a, b, return_games=True, **kw)
    two = arena.play_match(a, b, return_games=True, **kw)
    assert one == two
    ref = _drive(ids, S, None, 0)  # (test 2's games: base 10 gives parity 0)
    for g, game in zip(ids, one["games"]):
        assert game["game_id"] == g and game["moves"] == ref[g]["moves"]
        assert game["winner"] == (ref[g]["winner"] or None)
        assert game["color_a"] == (1 if MR.side_of(g, 1, 0) == 0 else 2)
    assert one["wins"] + one["losses"] + one["draws"] == 6 and one["win_rate"] == one["wins"] / 6
    assert one["wins"] == sum(1 for x in one["games"] if x["winner"] == x["color_a"])
    assert one["plies"] == sum(len(ref[g]["moves"]) for g in ids)
    assert one["wilson95"] == arena.wilson(one["wins"] + 0.5 * one["draws"], 6)
    ev = training.evaluate_model(a, b, games=6, eval_num_sim=S, seed=SEED, game_id_base=10, search="puct",
                                 puct={"c_puct": C_PUCT, "temp_plies": TEMP, "precision_a": "f16x3",
                                       "precision_b": "f16"})
    assert {k: ev[k] for k in ("wins", "losses", "draws", "win_rate")} == \
        {k: one[k] for k in ("wins", "losses", "draws", "win_rate")}
    # a match cut into steps of 1 ply and of 7 plies
    m1, m7 = _match(_sides(), 6, S, base=10), _match(_sides(), 6, S, base=10)
    m1.run(1)
    m7.run(7)
    (r1, v1), (r7, v7) = m1.records(), m7.records()
    assert r1.tobytes() == r7.tobytes() and v1.tobytes() == v7.tobytes() and m1.tally() == m7.tally()
    assert m7.steps < m1.steps
