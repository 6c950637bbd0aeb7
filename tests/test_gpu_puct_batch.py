"""Leaf batching with virtual loss on the GPU (GZ_PUCT_LEAF_BATCH; puct_select_batch_kernel
and puct_backup_batch_kernel of csrc/gz_puct.hip) against the plain-Python restatement in
tests/puct_batch_ref.py, bit for bit: whole trees and every round's rows through the step
API with synthetic evaluators, K = 1 against the unbatched search, gz_puct_search with
real weights, the root noise, self-play, the agent and the tree-reuse errors."""
import ctypes

import numpy as np
import pytest

import puct_batch_ref as B
import puct_noise_ref as NR
import puct_ref as R
from gzero import _lib, boards, device
from gzero.selfplay import SelfPlayEngine, records_to_games
from test_gpu_puct import C_PUCT, _assert_tree, _state, _thinned, _weights, make_synth

pytestmark = pytest.mark.gpu

SEED = 3


def _cells_of(rows):
    return boards.words_to_cells(rows[:, :8], rows[:, 8:])


def _flagged(S, K, temp_plies=0, seed=SEED, precision="f16x3", alpha=None, eps=0.25):
    """A gz_puct_batch_params with GZ_PUCT_LEAF_BATCH set, also at K = 1 (where
    device.puct_params would clear the flag): the batch kernels run."""
    mode = _lib.GZ_PV_FP32 if precision == "fp32" else _lib.GZ_PV_F16X3
    flags = _lib.GZ_PUCT_LEAF_BATCH | (_lib.GZ_PUCT_ROOT_NOISE if alpha is not None else 0)
    return _lib.PuctBatchParams(S, temp_plies, C_PUCT, seed, mode, flags, alpha or 0.0, eps if alpha is not None else 0.0,
                                K, 0)


def _tree_bytes(tree):
    return {k: np.asarray(v).tobytes() for k, v in tree.items()}


def _assert_rows(gpu, ref):
    """_assert_tree and every prior row of a live node, float64 bit for bit."""
    _assert_tree(gpu, ref)
    for k, t in enumerate(ref.term):
        if t == 0:
            assert [float(x) for x in gpu["prior"][k]] == list(ref.prior[k]), k


def _live_cells(s):
    return [int(x) for x in boards.words_to_cells(s["black"], s["white"])]


def _drive(states, gids, p, evals, noise=None):
    """The step API with host evaluators, the reference round by round beside it: every
    round's active mask and leaf boards, remaining() after every round, one more round that
    must change nothing, then finish.  Returns (refs, moves, visits, q, trees, rounds)."""
    n, S, K = len(states), p.num_simulations, p.leaves_per_round
    st = device.PuctStepper(states, gids, p)
    assert st.K == K and st.rows == n * K
    refs = [None if s["over"] else
            B.Search(_live_cells(s), int(s["player"]), int(s["n_moves"]), S, K, C_PUCT, evals[g],
                     None if noise is None else NR.Noise(SEED, gids[g], *noise))
            for g, s in enumerate(states)]
    rounds = 0
    while True:
        if rounds:
            st.select()
        rows, active = st.leaves()
        cells = _cells_of(rows)
        prior = np.zeros((n * K, 225), np.float64)
        value = np.zeros(n * K, np.float32)
        for g, ref in enumerate(refs):
            want = [None] * K if ref is None else ref.begin_round()
            results = []
            for k in range(K):
                r = g * K + k
                if want[k] is None:
                    assert not active[r] and not rows[r].any(), (rounds, g, k)
                else:
                    assert active[r] and tuple(int(x) for x in cells[r]) == want[k], (rounds, g, k)
                    prior[r], value[r] = evals[g](want[k], None)
                    results.append(([float(x) for x in prior[r]], float(value[r])))
            if ref is not None:
                ref.end_round(results)
        st.backup(prior, value)
        rounds += 1
        rem = st.remaining()
        assert list(rem) == [0 if ref is None else ref.remaining() for ref in refs], rounds
        if not rem.any():
            break
        assert rounds <= S + 1
    before = [_tree_bytes(t) for t in st.trees()]
    st.select()  # every game is at its budget: inactive rows, nothing changes
    rows, active = st.leaves()
    assert not active.any() and not rows.any()
    st.backup(np.ones((n * K, 225), np.float64), np.ones(n * K, np.float32))
    assert not st.remaining().any()
    moves, visits, q = st.finish()
    trees = st.trees()
    for g, t in enumerate(trees):
        tb = _tree_bytes(t)
        # (finish stores the move and its draw count)
        assert all(tb[k] == before[g][k] for k in tb if k not in ("move", "main_draws")), g
    for g, ref in enumerate(refs):
        if ref is None:
            assert moves[g] == -1 and not visits[g].any() and q[g] == 0.0
            continue
        _assert_rows(trees[g], ref.t)
        assert list(visits[g]) == ref.t.root_visits() and int(visits[g].sum()) == S
        mv, draws = R.choose_move(ref.t, p.temp_plies, SEED, int(gids[g]))
        assert int(moves[g]) == mv and trees[g]["move"] == mv and trees[g]["main_draws"] == draws
        assert float(q[g]) == R.root_q(ref.t)
        assert trees[g]["n_evals"] == ref.n_evals and trees[g]["n_nodes"] <= S + 1
    return refs, moves, visits, q, trees, rounds


# ---------------------------------------------------------------- 1. trees against the reference
PEAK = 100


def _six_games():
    """Three games at different plies (one of them over), then the crafted inputs: the
    peaked prior (collisions), the open four for the side to move and the blocked four
    (terminal backups inside a batch)."""
    sparse = np.zeros(225, np.int8)
    for c, x in ((112, 1), (113, 2), (97, 1), (128, 2), (111, 1), (127, 2), (96, 1)):
        sparse[c] = x
    tcells, tplayer, tmoves = R.tactical_position()
    bcells, bplayer, bmoves = B.blocked_four()
    states = np.concatenate([_state(_thinned(41, 1)), _state(_thinned(30, 2)), _state(_thinned(56, 3), over=1),
                             _state(sparse), _state(tcells, tmoves, tplayer), _state(bcells, bmoves, bplayer)])
    evals = [make_synth(), make_synth(boost=[224]), make_synth(), B.peaked_eval(PEAK), B.boosted_eval(112),
             B.boosted_eval((100, 112))]
    return states, [11, (1 << 40) + 3, 13, 14, 15, 16], evals


@pytest.mark.parametrize("S,K", [(24, 1), (24, 2), (24, 4), (24, 8), (7, 4), (3, 8)])
def test_step_api_trees_equal_the_reference(S, K):
    states, gids, evals = _six_games()
    refs, moves, visits, q, trees, rounds = _drive(states, gids, _flagged(S, K), evals)
    assert refs[2] is None
    live = [r for r in refs if r is not None]
    assert rounds == max(r.rounds for r in live) <= S + 1
    for r in live:
        assert 1 + -(-(S - r.terminal_sims) // K) <= r.rounds <= S + 1
        assert r.t.visits == r.through
    # the counters on the reference itself: the crafted inputs do what they were made for
    if K >= 2 and S >= 2:
        assert refs[3].collisions >= 1 and trees[3]["move_of"][1] == PEAK
    assert refs[4].batch_terminals >= 1 and refs[4].terminal_sims == S and trees[4]["term"][1] == 1
    assert refs[4].rounds == 2
    if S >= 24:
        assert refs[5].batch_terminals >= 1 and 0 < refs[5].terminal_sims < S
        assert max(r.t.count[k] - r.t.count[0] for r in live for k in range(len(r.t.parent))) >= 2  # depth > 1


@pytest.mark.parametrize("K", [0, 3])
def test_a_select_without_the_backup_before_it_changes_nothing(K):
    """A node still waits for its evaluation (header.pending): the select step leaves every
    row inactive and empty and every tree byte as it was.  K = 0 is the flag-clear search
    (puct_select_kernel), where the root and every later leaf wait that way; with leaf
    batching only the root does."""
    S = 4
    states = np.concatenate([_state(_thinned(41, 1)), _state(_thinned(30, 2))])
    evals = [make_synth(), make_synth()]
    st = device.PuctStepper(states, [11, 12], _flagged(S, K) if K else device.puct_params(S, C_PUCT, 0, SEED))
    per = max(K, 1)

    def select_again():
        before = [_tree_bytes(t) for t in st.trees()]
        st.select()
        rows, active = st.leaves()
        assert not active.any() and not rows.any()
        assert [_tree_bytes(t) for t in st.trees()] == before

    rows, active = st.leaves()
    assert list(np.flatnonzero(active)) == [0, per]  # the two roots
    select_again()
    if K:
        return
    prior = np.zeros((2, 225), np.float64)
    value = np.zeros(2, np.float32)
    for g in range(2):
        prior[g], value[g] = evals[g](_cells_of(rows)[g], None)
    st.backup(prior, value)
    st.select()
    assert st.leaves()[1].all() and [t["n_nodes"] for t in st.trees()] == [2, 2]
    select_again()  # the new leaves wait


# ---------------------------------------------------------------- 2. K = 1 leaves today's path alone
def _five_states():
    tcells, tplayer, tmoves = R.tactical_position()
    return np.concatenate([_state(np.zeros(225, np.int8)), _state(_thinned(12, 7)), _state(_thinned(47, 8)),
                           _state(tcells, tmoves, tplayer), _state(_thinned(200, 9))])


def test_one_leaf_per_round_equals_the_flag_clear_search():
    w = _weights("f16x3")
    S, gids = 24, [20, 21, 22, 23, 24]
    states = _five_states()
    plain = device.puct_search(states, gids, device.puct_params(S, C_PUCT, 0, 9), w, want_trees=True)
    assert type(device.puct_params(S, C_PUCT, 0, 9, leaves_per_round=1)) is _lib.PuctParams
    flagged = device.puct_search(states, gids, _flagged(S, 1, seed=9), w, want_trees=True)
    for a, b in zip(plain[:3], flagged[:3]):
        assert a.tobytes() == b.tobytes()
    for ta, tb in zip(plain[3], flagged[3]):
        assert _tree_bytes(ta) == _tree_bytes(tb)
    # and the keyword on device.puct_search
    again = device.puct_search(states, gids, device.puct_params(S, C_PUCT, 0, 9), w, want_trees=True,
                               leaves_per_round=1)
    assert all(_tree_bytes(ta) == _tree_bytes(tb) for ta, tb in zip(plain[3], again[3]))


# ---------------------------------------------------------------- 3. real weights
def _table_eval(tree):
    cells = _cells_of(tree["board"])
    table = {tuple(int(x) for x in cells[k]): ([float(x) for x in tree["prior"][k]], float(tree["value"][k]))
             for k in range(tree["n_nodes"]) if tree["term"][k] == 0}

    def evalf(c, player):
        assert tuple(c) in table, "the reference asks for a board the GPU tree lacks"
        return table[tuple(c)]

    return evalf


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_search_with_real_weights(precision):
    w = _weights(precision)
    S, K, n = 16, 4, 5
    states, gids = _five_states(), [20, 21, 22, 23, 24]
    p = device.puct_params(S, C_PUCT, 0, 9, precision, leaves_per_round=K)
    moves, visits, q, trees = device.puct_search(states, gids, p, w, want_trees=True)
    # every stored prior row and value = the standalone forward of that node's board (rows
    # are independent: no tolerance)
    rows = np.concatenate([t["board"][t["term"] == 0] for t in trees])
    prior = np.concatenate([t["prior"][t["term"] == 0] for t in trees])
    value = np.concatenate([t["value"][t["term"] == 0] for t in trees])
    _, fv, _, fprior = device.pv_forward(w, rows, want_prior=True)
    assert np.array_equal(prior, fprior) and np.array_equal(value, fv)
    # the reference driven by those values builds the same trees
    for g in range(n):
        s = states[g]
        ref = B.search(_live_cells(s), int(s["player"]), int(s["n_moves"]), S, K, C_PUCT, _table_eval(trees[g]))
        _assert_rows(trees[g], ref.t)
        assert list(visits[g]) == ref.t.root_visits() and visits[g].sum() == S
        assert int(moves[g]) == R.choose_move(ref.t, 0, 9, gids[g])[0]
        assert float(q[g]) == R.root_q(ref.t)
        assert trees[g]["n_evals"] == ref.n_evals
    # the keyword on device.puct_search is the same search
    m2, v2, q2, _ = device.puct_search(states, gids, device.puct_params(S, C_PUCT, 0, 9, precision), w,
                                       leaves_per_round=K)
    assert np.array_equal(m2, moves) and np.array_equal(v2, visits) and np.array_equal(q2, q)


# ---------------------------------------------------------------- 4. root noise
def test_root_noise_with_batching():
    S, K, alpha, eps = 24, 4, 0.3, 0.25
    states = np.concatenate([_state(_thinned(41, 1)), _state(_thinned(30, 2)), _state(np.zeros(225, np.int8))])
    gids = [11, (1 << 40) + 3, 13]
    evals = [make_synth(), make_synth(boost=[224]), make_synth()]
    refs, _, _, _, trees, _ = _drive(states, gids, _flagged(S, K, alpha=alpha, eps=eps), evals, noise=(alpha, eps))
    for g, s in enumerate(states):
        cells = _live_cells(s)
        raw = evals[g](tuple(cells), None)[0]
        want = NR.mix(raw, cells, SEED, gids[g], int(s["n_moves"]), alpha, eps)
        assert [float(x) for x in trees[g]["prior"][0]] == want and want != raw
    # eps = 0 with the noise flag set is the noise-free batched tree, byte for byte
    zero = _drive(states, gids, _flagged(S, K, alpha=alpha, eps=0.0), evals, noise=(alpha, 0.0))
    off = _drive(states, gids, _flagged(S, K), evals)
    for a, b in zip(zero[1:4], off[1:4]):
        assert a.tobytes() == b.tobytes()
    assert [_tree_bytes(t) for t in zero[4]] == [_tree_bytes(t) for t in off[4]]


# ---------------------------------------------------------------- 5. self-play
ENG = dict(S=16, K=4, seed=21, temp=4, games=4)
_PLAYED = {}


def _play(n_slots):
    """Games 0..3 -> (records sorted by (id, ply), their visit rows, ids in finishing order)."""
    if n_slots not in _PLAYED:
        eng = SelfPlayEngine(n_slots=n_slots, num_simulations=ENG["S"], c_puct=C_PUCT, seed=ENG["seed"],
                             pv_weights=_weights("f16x3"), search="puct", temp_plies=ENG["temp"],
                             leaves_per_round=ENG["K"])
        recs, vis, done = [], [], []
        for _ in range(ENG["games"] // n_slots * 200 + 2):
            eng.step()
            c = eng.counters()
            assert c["records_dropped"] == 0 and c["moves"] == n_slots
            if c["records"]:
                r, v = eng.records().copy(), eng.visits().copy()
                keep = r["game_id"] < ENG["games"]
                recs.append(r[keep])
                vis.append(v[keep])
                done += [g for g in dict.fromkeys(int(x) for x in r["game_id"][keep]) if g not in done]
            if len(done) == ENG["games"]:
                break
        assert len(done) == ENG["games"]
        recs, vis = np.concatenate(recs), np.concatenate(vis)
        order = np.lexsort((recs["ply"], recs["game_id"]))
        _PLAYED[n_slots] = (recs[order], vis[order], done)
    return _PLAYED[n_slots]


def test_selfplay_equals_a_replay_through_the_reference():
    S, K = ENG["S"], ENG["K"]
    recs, vis, done = _play(4)
    assert (vis.astype(np.int64).sum(axis=1) == S).all()  # every visit row sums to S
    games = records_to_games(recs)
    w = _weights("f16x3")
    # the first two games that finished: one reference search per ply, all of them driven
    # together so that a round of all searches is one forward
    plies = []
    for gid in done[:2]:
        cells = [0] * 225
        for k, m in enumerate(games[gid]["moves"]):
            assert tuple(int(x) for x in games[gid]["cells"][k]) == tuple(cells)
            plies.append((gid, k, m, B.Search(list(cells), 1 + k % 2, k, S, K, C_PUCT, None)))
            cells[m] = 1 + k % 2
    assert len(plies) >= 2 * 9
    while True:
        asks = [(s, [r for r in s.begin_round() if r is not None]) for _, _, _, s in plies if s.remaining() > 0]
        if not asks:
            break
        flat = np.array([r for _, rows in asks for r in rows], np.int8).reshape(-1, 225)
        fprior, fv = np.zeros((0, 225)), np.zeros(0, np.float32)
        if len(flat):
            _, fv, _, fprior = device.pv_forward(w, boards.leaf_words(*boards.cells_to_words(flat)), want_prior=True)
        at = 0
        for s, rows in asks:
            s.end_round([([float(x) for x in fprior[at + i]], float(fv[at + i])) for i in range(len(rows))])
            at += len(rows)
    for gid, k, m, s in plies:
        row = vis[recs["game_id"] == gid][k]
        assert list(row.astype(np.int64)) == s.t.root_visits(), (gid, k)
        assert R.choose_move(s.t, ENG["temp"], ENG["seed"], gid)[0] == m, (gid, k)
        assert 1 + -(-(S - s.terminal_sims) // K) <= s.rounds <= S + 1


def test_selfplay_games_do_not_depend_on_the_slot_count():
    a, b = _play(4), _play(2)
    assert len(a[0]) == len(b[0]) and a[0].tobytes() == b[0].tobytes()
    assert np.array_equal(a[1], b[1])


# ---------------------------------------------------------------- 6. the agent
def test_ai_agent_with_leaf_batching():
    from ai_agent import AIFactory
    from gomoku_board import GomokuBoard
    ai = AIFactory.create_ai("alphazero", 1, "easy", search="puct", seed=5, game_id=2, leaves_per_round=4)
    b0, b1 = GomokuBoard(), GomokuBoard()
    for r, c in ((7, 7), (7, 8), (8, 8)):
        b1.make_move(r, c)
    got = ai.get_moves([b0, b1], [2, 9])
    S = ai.params["num_simulations"]
    assert ai.last_search_visits.shape == (2, 225) and list(ai.last_search_visits.sum(axis=1)) == [S, S]
    assert ai.last_root_value.shape == (2,) and np.all(np.abs(ai.last_root_value) <= 1.0)
    p = device.puct_params(S, ai.params["c_puct"], 0, 5, leaves_per_round=4)
    states = np.concatenate([b0.to_state(), b1.to_state()])
    mv, visits, q, _ = device.puct_search(states, [2, 9], p, ai.model.device_weights())
    assert got == [(int(m) // 15, int(m) % 15) for m in mv]
    assert np.array_equal(visits, ai.last_search_visits) and np.array_equal(q, ai.last_root_value)
    assert ai.get_move(b0) == got[0]


# ---------------------------------------------------------------- 7. errors
def test_tree_reuse_with_leaf_batching_is_refused():
    with pytest.raises(ValueError):
        SelfPlayEngine(n_slots=4, num_simulations=8, pv_weights=_weights("f16x3"), search="puct", tree_reuse=True,
                       leaves_per_round=4)
    st = device.PuctStepper(_five_states()[:2], [0, 1], device.puct_params(8, C_PUCT, leaves_per_round=4))
    with pytest.raises(_lib.GzeroError, match="leaves_per_round > 1 is not supported"):
        st.reroot([-1, -1])
    # the library's own check of the self-play entry point (before any launch)
    eng = SelfPlayEngine(n_slots=2, num_simulations=8, pv_weights=_weights("f16x3"), search="puct", leaves_per_round=4)
    with pytest.raises(_lib.GzeroError, match="leaves_per_round > 1 is not supported"):
        eng._puct_rounds(1)
    # K = 1 re-roots as before
    one = device.PuctStepper(_five_states()[:2], [0, 1], device.puct_params(8, C_PUCT))
    assert list(one.reroot([-1, -1])) == [9, 9]
