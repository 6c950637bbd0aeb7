"""The PUCT mode with precision="f16" (GZ_PV_F16 leaf evaluations): gz_puct_search,
lock-step self-play, tree reuse, leaf batching and the training switch
(selfplay_precision) -- each against the same run driven from Python with the
standalone gz_pv_forward(GZ_PV_F16) as the evaluator, bit for bit."""
import random

import numpy as np
import pytest
import torch

import puct_batch_ref as B
import puct_ref as R
from gzero import _lib, boards, device, weights
from gzero.boards import RECORD_DTYPE
from gzero.selfplay import SelfPlayEngine, records_to_games
from test_gpu_puct import C_PUCT, _assert_tree, _replay, _state, _thinned

pytestmark = pytest.mark.gpu

ENG = dict(S=8, slots=4, temp=4, seed=21, games=4)
_W = {}


def _w16():
    if "w" not in _W:
        _W["w"] = device.PVWeights(weights.pack_pv_weights(weights.init_state_dict(0)), precision="f16")
    return _W["w"]


def _standalone_eval():
    """evalf(cells, player) = the standalone F16 forward of that one board."""
    cache = {}

    def evalf(cells, player):
        key = tuple(int(x) for x in cells)
        if key not in cache:
            rows = boards.leaf_words(*boards.cells_to_words(np.array(key, np.int8)[None]))
            _, v, _, prior = device.pv_forward(_w16(), rows, want_prior=True)
            cache[key] = ([float(x) for x in prior[0]], float(v[0]))
        return cache[key]

    return evalf


# ---------------------------------------------------------------- 1. gz_puct_search
def test_search_f16_equals_the_reference_on_the_standalone_forward():
    w = _w16()
    assert w.mode == _lib.GZ_PV_F16
    S, gids = 12, [20, 21, 22]
    states = np.concatenate([_state(np.zeros(225, np.int8)), _state(_thinned(12, 7)), _state(_thinned(47, 8))])
    p = device.puct_params(S, C_PUCT, 0, 9, "f16")
    assert p.precision == _lib.GZ_PV_F16
    moves, visits, q, trees = device.puct_search(states, gids, p, w, want_trees=True)
    evalf = _standalone_eval()
    for g, s in enumerate(states):
        cells = boards.words_to_cells(s["black"], s["white"])
        ref = R.search([int(x) for x in cells], int(s["player"]), int(s["n_moves"]), S, C_PUCT, evalf)
        _assert_tree(trees[g], ref)
        for k, t in enumerate(ref.term):
            if t == 0:
                assert [float(x) for x in trees[g]["prior"][k]] == list(ref.prior[k]), (g, k)
        assert list(visits[g]) == ref.root_visits() and visits[g].sum() == S
        assert int(moves[g]) == R.choose_move(ref, 0, 9, gids[g])[0]
        assert float(q[g]) == R.root_q(ref)
    # every stored prior row and value = the standalone forward's bytes (all nodes in one call)
    rows = np.concatenate([t["board"][t["term"] == 0] for t in trees])
    prior = np.concatenate([t["prior"][t["term"] == 0] for t in trees])
    value = np.concatenate([t["value"][t["term"] == 0] for t in trees])
    _, fv, _, fprior = device.pv_forward(w, rows, want_prior=True)
    assert prior.tobytes() == fprior.tobytes() and value.tobytes() == fv.tobytes()
    # ... and they are F16's, not f16x3's
    w3 = device.PVWeights(weights.pack_pv_weights(weights.init_state_dict(0)), precision="f16x3")
    assert not np.array_equal(device.pv_forward(w3, rows, want_prior=True)[3], fprior)


# ---------------------------------------------------------------- 2. self-play
def _engine_games(**kw):
    """Games 0..3 on a 4-slot F16 engine -> (records sorted by (id, ply), visit rows)."""
    eng = SelfPlayEngine(n_slots=ENG["slots"], num_simulations=ENG["S"], c_puct=C_PUCT, seed=ENG["seed"],
                         pv_weights=_w16(), search="puct", temp_plies=ENG["temp"], **kw)
    assert eng.puct.precision == _lib.GZ_PV_F16
    recs, vis, done = [], [], set()
    for _ in range(200 * (ENG["S"] + 1) + 2):
        eng.step()
        c = eng.counters()
        assert c["records_dropped"] == 0
        if c["records"]:
            r, v = eng.records().copy(), eng.visits().copy()
            keep = r["game_id"] < ENG["games"]
            recs.append(r[keep])
            vis.append(v[keep])
            done |= set(int(x) for x in r["game_id"][keep])
        if len(done) == ENG["games"]:
            break
    assert len(done) == ENG["games"]
    recs, vis = np.concatenate(recs), np.concatenate(vis)
    order = np.lexsort((recs["ply"], recs["game_id"]))
    return recs[order], vis[order]


def _forward_backup(st, n, bufs):
    _, d_value, _ = device.pv_forward_dev(_w16(), st.d_leaves, n, d_probs=bufs[0], d_prior=bufs[1])
    st.backup(bufs[1], d_value)


def _assert_games(recs, vis, driven):
    """driven: per game id (moves, visit rows) -> the records' moves, rows and z."""
    games = records_to_games(recs)
    assert sorted(games) == sorted(driven)
    for gid, (moves, rows) in driven.items():
        assert games[gid]["moves"] == moves, gid
        assert np.array_equal(vis[recs["game_id"] == gid].astype(np.int32), np.array(rows)), gid
        _, winner, over = _replay(moves)
        assert over, gid
        assert games[gid]["z"] == [0 if winner == 0 else (1 if 1 + k % 2 == winner else -1) for k in range(len(moves))]


def test_lockstep_selfplay_f16_equals_the_step_api():
    """4 slots x 8 simulations: a fresh search per ply.  The same games through PuctStepper,
    one stepper per ply over the games still running, the standalone F16 forward as the
    evaluator."""
    S, n = ENG["S"], ENG["games"]
    recs, vis = _engine_games()
    p = device.puct_params(S, C_PUCT, ENG["temp"], ENG["seed"], "f16")
    cells = np.zeros((n, 225), np.int8)
    driven = {g: ([], []) for g in range(n)}
    live = list(range(n))
    for ply in range(200):
        states = np.concatenate([_state(cells[g], ply, 1 + ply % 2) for g in live])
        st = device.PuctStepper(states, live, p)
        bufs = (torch.empty(len(live) * 225, dtype=torch.float32, device="cuda"),
                torch.empty(len(live) * 225, dtype=torch.float64, device="cuda"))
        for rnd in range(S + 1):
            if rnd:
                st.select()
            _forward_backup(st, len(live), bufs)
        moves, visits, _ = st.finish()
        nxt = []
        for i, g in enumerate(live):
            m = int(moves[i])
            driven[g][0].append(m)
            driven[g][1].append(visits[i].copy())
            cells[g][m] = 1 + ply % 2
            if not _replay(driven[g][0])[2]:
                nxt.append(g)
        live = nxt
        if not live:
            break
    _assert_games(recs, vis, driven)


def test_tree_reuse_selfplay_f16_equals_the_step_api():
    """The same 4 games with tree reuse: PuctStepper + reroot with the standalone forward."""
    S, n = ENG["S"], ENG["games"]
    recs, vis = _engine_games(tree_reuse=True, game_id_end=n)
    p = device.puct_params(S, C_PUCT, ENG["temp"], ENG["seed"], "f16")
    st = device.PuctStepper(np.concatenate([_state(np.zeros(225, np.int8))] * n), list(range(n)), p)
    bufs = (torch.empty(n * 225, dtype=torch.float32, device="cuda"),
            torch.empty(n * 225, dtype=torch.float64, device="cuda"))
    driven = {g: ([], []) for g in range(n)}
    _forward_backup(st, n, bufs)
    remaining = np.full(n, S)
    for ply in range(200):
        for _ in range(int(remaining.max())):
            st.select()
            _forward_backup(st, n, bufs)
        moves, visits, _ = st.finish()
        if (moves < 0).all():
            break
        for g in range(n):
            if moves[g] >= 0:
                driven[g][0].append(int(moves[g]))
                driven[g][1].append(visits[g].copy())
        remaining = st.reroot(moves)
    _assert_games(recs, vis, driven)


def test_leaf_batching_selfplay_f16_equals_the_reference():
    """K = 4 leaves per round: every ply of the first two games replayed through
    tests/puct_batch_ref.py with the standalone F16 forward (a round of all the searches is
    one forward)."""
    S, K = ENG["S"], 4
    recs, vis = _engine_games(leaves_per_round=K)
    assert (vis.astype(np.int64).sum(axis=1) == S).all()
    games = records_to_games(recs)
    plies = []
    for gid in (0, 1):
        cells = [0] * 225
        for k, m in enumerate(games[gid]["moves"]):
            plies.append((gid, k, m, B.Search(list(cells), 1 + k % 2, k, S, K, C_PUCT, None)))
            cells[m] = 1 + k % 2
        _, winner, over = _replay(games[gid]["moves"])
        assert over and games[gid]["z"] == [0 if winner == 0 else (1 if 1 + k % 2 == winner else -1)
                                            for k in range(len(games[gid]["moves"]))]
    while True:
        asks = [(s, [r for r in s.begin_round() if r is not None]) for _, _, _, s in plies if s.remaining() > 0]
        if not asks:
            break
        flat = np.array([r for _, rows in asks for r in rows], np.int8).reshape(-1, 225)
        fprior, fv = np.zeros((0, 225)), np.zeros(0, np.float32)
        if len(flat):
            _, fv, _, fprior = device.pv_forward(_w16(), boards.leaf_words(*boards.cells_to_words(flat)),
                                                 want_prior=True)
        at = 0
        for s, rows in asks:
            s.end_round([([float(x) for x in fprior[at + i]], float(fv[at + i])) for i in range(len(rows))])
            at += len(rows)
    for gid, k, m, s in plies:
        row = vis[recs["game_id"] == gid][k]
        assert list(row.astype(np.int64)) == s.t.root_visits(), (gid, k)
        assert R.choose_move(s.t, ENG["temp"], ENG["seed"], gid)[0] == m, (gid, k)


# ---------------------------------------------------------------- 3. training
def test_run_iteration_with_selfplay_precision_f16(monkeypatch):
    """run_iteration(search="puct", selfplay_precision="f16") on an f16x3 model: it completes,
    its self-play records and visit rows are those of selfplay_puct_device on an "f16"
    PVWeights of the same parameters, and the model's own weights stay f16x3."""
    import training
    from gzero.train import DeviceTrainer
    from neural_network import GomokuModel

    def model7():
        m = GomokuModel(device="cpu")
        m.model.load_state_dict(weights.init_state_dict(seed=7))
        return m

    model = model7()
    trainer = DeviceTrainer(model)
    assert model.device_weights().precision == "f16x3"
    own = model.device_weights()
    second = model.device_weights("f16")
    assert second.precision == "f16" and second is model.device_weights("f16") and own is model.device_weights()
    seen = {}
    real = training.selfplay_puct_device

    def spy(*a, **k):
        out = real(*a, **k)
        seen["weights"] = k["pv_weights"]
        seen["recs"] = out[0][:out[2]].cpu().numpy().copy()
        seen["vis"] = out[1][:out[2]].cpu().numpy().copy()
        return out

    monkeypatch.setattr(training, "selfplay_puct_device", spy)
    random.seed(123)
    torch.manual_seed(456)
    res = training.run_iteration(model, trainer, 3, games_per_iteration=2, num_simulations=8, batch_size=32, epochs=1,
                                 seed=11, search="puct", verbose=False, selfplay_precision="f16")
    monkeypatch.undo()
    assert seen["weights"] is second and not res.get("skipped")
    assert np.isfinite(res["train_loss"]) and np.isfinite(res["val_loss"]) and res["records"] == len(seen["recs"])
    # the SGD moved the parameters: both packs follow, each at its own precision
    assert model.device_weights().precision == "f16x3" and model.device_weights() is not own
    assert model.device_weights("f16") is not second and model.precision == "f16x3"

    again = model7()
    DeviceTrainer(again)
    w16 = device.PVWeights(weights.pack_pv_weights_torch(again.model.state_dict(), "cuda"), precision="f16")
    d, d_vis, n, _ = training.selfplay_puct_device(2, num_simulations=8, seed=11, game_id_base=6, model=again,
                                                   temp_plies=8, pv_weights=w16)
    assert n == res["records"] >= 2 * 9
    assert d[:n].cpu().numpy().tobytes() == seen["recs"].tobytes()
    assert np.array_equal(d_vis[:n].cpu().numpy(), seen["vis"])
    recs = np.frombuffer(seen["recs"].tobytes(), RECORD_DTYPE)
    assert sorted(set(int(g) for g in recs["game_id"])) == [6, 7]
    with pytest.raises(ValueError, match="selfplay_precision"):
        training.run_iteration(model, trainer, 0, selfplay_precision="f16")
