"""The network-guided PUCT search on the GPU (csrc/gz_puct.hip) against the plain-
Python restatement in tests/puct_ref.py: whole trees through the step API with a
synthetic evaluator, gz_puct_search with real weights, move sampling, self-play."""
import numpy as np
import pytest
import torch

import puct_ref as R
from conftest import SEED, golden
from gzero import boards, device, rng, weights
from gzero.selfplay import SelfPlayEngine, records_to_games

pytestmark = pytest.mark.gpu

C_PUCT = 1.6


# ---------------------------------------------------------------- evaluators
def _board_hash(cells):
    h = 0
    for c, x in enumerate(cells):
        if x:
            h = rng.mix64(h ^ (c * 4 + x))
    return h


def make_synth(boost=(), weight=10.0, flat=False):
    """evalf(cells, player): prior weights mix64(board hash ^ cell) in [0, 1) (or all
    1 with flat), plus `weight` at the cells of `boost`, masked and normalised with a
    float64 numpy sum; value a float32 in (-1, 1) from the hash."""
    cache = {}

    def evalf(cells, player):
        cells = tuple(int(x) for x in cells)
        if cells not in cache:
            h = _board_hash(cells)
            if flat:
                w = np.ones(225, np.float64)
            else:
                w = np.array([(rng.mix64(h ^ c) >> 11) * (1.0 / 9007199254740992.0) for c in range(225)], np.float64)
            for c in boost:
                w[c] += weight
            w = w * (np.array(cells) == 0)
            prior = w / np.sum(w)
            v = np.float32(((rng.mix64(h ^ 0xABCDEF) >> 40) / float(1 << 24)) * 1.9 - 0.95)
            cache[cells] = ([float(x) for x in prior], float(v))
        return cache[cells]

    return evalf


def _uniform(cells, player):
    return R.uniform_eval(list(cells), player)


# ---------------------------------------------------------------- positions
def _pattern_cells():
    """A full board with no run longer than two in any direction."""
    return np.array([1 + ((c // 2 + r) % 2) for r in range(15) for c in range(15)], np.int8)


def _thinned(keep, seed):
    cells = _pattern_cells()
    drop = np.random.RandomState(seed).permutation(225)[keep:]
    cells[drop] = 0
    return cells


def _state(cells, n_moves=None, player=None, over=0):
    cells = np.asarray(cells, np.int8)
    stones = int((cells != 0).sum())
    n_moves = stones if n_moves is None else n_moves
    player = 1 + n_moves % 2 if player is None else player
    return boards.make_states(cells[None], n_moves=n_moves, player=player, over=over)


# ---------------------------------------------------------------- drivers
def _run_steps(states, gids, S, evals, temp_plies=0, seed=3):
    """The step API with per-game host evaluators; returns (moves, visits, q, trees)."""
    n = len(states)
    p = device.puct_params(S, C_PUCT, temp_plies, seed)
    st = device.PuctStepper(states, gids, p)
    players = {}
    for rnd in range(S + 1):
        if rnd:
            st.select()
        rows, active = st.leaves()
        cells = boards.words_to_cells(rows[:, :8], rows[:, 8:])
        prior = np.zeros((n, 225), np.float64)
        value = np.zeros(n, np.float32)
        for g in range(n):
            if active[g]:
                pr, v = evals[g](cells[g], players.get(g))
                prior[g], value[g] = pr, v
            else:
                assert not rows[g].any(), "a game without a leaf leaves an empty board"
        st.backup(prior, value)
    moves, visits, q = st.finish()
    return moves, visits, q, st.trees()


def _assert_tree(gpu, ref):
    k = len(ref.parent)
    assert gpu["n_nodes"] == k
    assert list(gpu["parent"]) == ref.parent
    assert list(gpu["move_of"]) == ref.move
    assert list(gpu["term"]) == ref.term
    assert list(gpu["visits"]) == ref.visits
    assert [float(x) for x in gpu["W"]] == ref.W  # float64, bit for bit
    assert [float(x) for x in gpu["value"]] == ref.value
    cells = boards.words_to_cells(gpu["board"][:, :8], gpu["board"][:, 8:])
    assert [tuple(int(x) for x in row) for row in cells] == ref.cells
    assert gpu["n_evals"] == sum(1 for t in ref.term if t == 0)


def _check_games(states, gids, S, evals, temp_plies=0, seed=3):
    moves, visits, q, trees = _run_steps(states, gids, S, evals, temp_plies, seed)
    refs = []
    for g in range(len(states)):
        s = states[g]
        if s["over"]:
            assert moves[g] == -1 and not visits[g].any() and q[g] == 0.0
            refs.append(None)
            continue
        cells = boards.words_to_cells(s["black"], s["white"])
        ref = R.search([int(x) for x in cells], int(s["player"]), int(s["n_moves"]), S, C_PUCT, evals[g])
        _assert_tree(trees[g], ref)
        assert list(visits[g]) == ref.root_visits()
        mv, draws = R.choose_move(ref, temp_plies, seed, int(gids[g]))
        assert int(moves[g]) == mv and trees[g]["move"] == mv
        assert trees[g]["main_draws"] == draws
        assert float(q[g]) == R.root_q(ref)
        refs.append(ref)
    return moves, visits, refs


# ---------------------------------------------------------------- 1. step API
@pytest.mark.parametrize("S", [1, 2, 120])
def test_step_api_trees_equal_the_reference(S):
    # game 1: cell 224 has the largest prior; game 2: cells 192..224 the top priors
    # (both live in the last, partial lane chunk)
    states = np.concatenate([_state(_thinned(41, 1)), _state(_thinned(30, 2)), _state(_thinned(56, 3))])
    for s in states:
        cells = boards.words_to_cells(s["black"], s["white"])
        assert (cells[192:] == 0).sum() >= 20
    states[1]["black"], states[1]["white"] = boards.cells_to_words(_clear(_thinned(30, 2), [224]))
    evals = [make_synth(), make_synth(boost=[224]), make_synth(boost=range(192, 225))]
    moves, visits, refs = _check_games(states, [11, 12, 13], S, evals)
    assert visits[1][224] >= 1
    assert visits[2][192:].sum() >= min(S, 20) and visits[2].sum() == S


def _clear(cells, which):
    cells = np.array(cells, np.int8)
    cells[list(which)] = 0
    return cells


def test_step_api_ties_and_the_tactical_position():
    # game 0: two cells share the bit-equal top prior, so the first wins every tie;
    # game 1: the tactical position with the uniform prior (every score ties at first);
    # game 2: the empty board
    tie = _clear(_thinned(40, 4), [37, 100])
    tcells, tplayer, tmoves = R.tactical_position()
    states = np.concatenate([_state(tie), _state(tcells, tmoves, tplayer), _state(np.zeros(225, np.int8))])
    evals = [make_synth(boost=[37, 100], weight=5.0, flat=True), _uniform, make_synth()]
    moves, visits, refs = _check_games(states, [0, 1, 2], 120, evals)
    pr = refs[0].prior[0]
    assert pr[37] == pr[100] == max(pr)
    first = refs[0].move[1]
    assert first == 37
    assert int(moves[1]) == 107 and visits[1][107] == 15 and visits[1][112] == 0
    assert len(refs[1].parent) == 107 and sorted(set(visits[1])) == [0, 1, 15]


def test_step_api_late_positions_at_300_simulations():
    late = _thinned(185, 5)                       # 40 empties: deep trees, the 200-ply cap in reach
    one = _clear(_pattern_cells(), [113])         # one empty cell: the root's only child is terminal
    tcells, tplayer, _ = R.tactical_position()
    states = np.concatenate([_state(late), _state(one, n_moves=190), _state(tcells, 198, tplayer),
                             _state(_thinned(50, 6), over=1)])
    assert (boards.words_to_cells(states[0]["black"], states[0]["white"]) == 0).sum() == 40
    evals = [make_synth(), make_synth(), make_synth(), make_synth()]
    moves, visits, refs = _check_games(states, [5, 6, 7, 8], 300, evals)
    assert refs[0].visits[0] == 301 and max(refs[0].count) >= 185 + 3
    assert len(refs[1].parent) == 2 and refs[1].visits[1] == 300 and int(moves[1]) == 113
    # black's fives and the 200-ply draw of every grandchild, revisited
    assert set(refs[2].term) <= {0, 1, 3} and 3 in refs[2].term and max(refs[2].count) == 200
    assert max(v for v, t in zip(refs[2].visits, refs[2].term) if t) > 1
    assert int(moves[3]) == -1


# ---------------------------------------------------------------- 2. real weights
_W = {}


def _weights(precision):
    if precision not in _W:
        _W[precision] = device.PVWeights(weights.pack_pv_weights(weights.init_state_dict(0)), precision)
    return _W[precision]


def _five_states():
    tcells, tplayer, tmoves = R.tactical_position()
    return np.concatenate([_state(np.zeros(225, np.int8)), _state(_thinned(12, 7)), _state(_thinned(47, 8)),
                           _state(tcells, tmoves, tplayer), _state(_thinned(200, 9))])


@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_search_with_real_weights(precision):
    w = _weights(precision)
    S, n = 64, 5
    states, gids = _five_states(), [20, 21, 22, 23, 24]
    p = device.puct_params(S, C_PUCT, 0, 9, precision)
    moves, visits, q, trees = device.puct_search(states, gids, p, w, want_trees=True)

    # the reference replayed with the tree's own (board -> prior, value) reproduces it
    for g in range(n):
        t = trees[g]
        cells = boards.words_to_cells(t["board"][:, :8], t["board"][:, 8:])
        table = {tuple(int(x) for x in cells[k]): ([float(x) for x in t["prior"][k]], float(t["value"][k]))
                 for k in range(t["n_nodes"]) if t["term"][k] == 0}

        def evalf(c, player, table=table):
            assert tuple(c) in table, "the reference asks for a board the GPU tree lacks"
            return table[tuple(c)]

        s = states[g]
        ref = R.search([int(x) for x in cells[0]], int(s["player"]), int(s["n_moves"]), S, C_PUCT, evalf)
        _assert_tree(t, ref)
        assert list(visits[g]) == ref.root_visits() and visits[g].sum() == S
        assert int(moves[g]) == R.choose_move(ref, 0, 9, gids[g])[0]
        assert float(q[g]) == R.root_q(ref)

    # every node's stored prior and value = a standalone forward of the exported boards
    rows = np.concatenate([t["board"][t["term"] == 0] for t in trees])
    prior = np.concatenate([t["prior"][t["term"] == 0] for t in trees])
    value = np.concatenate([t["value"][t["term"] == 0] for t in trees])
    _, fv, _, fprior = device.pv_forward(w, rows, want_prior=True)
    print(f"{precision}: {len(rows)} nodes, max |dprior| {np.abs(prior - fprior).max():.3e}, "
          f"max |dvalue| {np.abs(value - fv).max():.3e}")
    assert np.array_equal(prior, fprior) and np.array_equal(value, fv)

    # the same search driven through the step API with gz_pv_forward as the evaluator
    st = device.PuctStepper(states, gids, p)
    d_probs = torch.empty(n * 225, dtype=torch.float32, device="cuda")
    d_prior = torch.empty(n * 225, dtype=torch.float64, device="cuda")
    for rnd in range(S + 1):
        if rnd:
            st.select()
        _, d_value, _ = device.pv_forward_dev(w, st.d_leaves, n, d_probs=d_probs, d_prior=d_prior)
        st.backup(d_prior, d_value)
    m2, v2, q2 = st.finish()
    assert np.array_equal(m2, moves) and np.array_equal(v2, visits) and np.array_equal(q2, q)
    for a, b in zip(st.trees(), trees):
        assert a["n_nodes"] == b["n_nodes"]
        for key in ("W", "visits", "value", "parent", "move_of", "term", "board"):
            assert np.array_equal(a[key], b[key]), key
        live = a["term"] == 0
        assert np.array_equal(a["prior"][live], b["prior"][live])


# ---------------------------------------------------------------- 3. move sampling
def test_move_sampling():
    w = _weights("f16x3")
    S, n, seed = 32, 8, 77
    cells = _thinned(10, 10)
    states = np.concatenate([_state(cells)] * n)
    gids = [3, 1000, 17, 4, 5, 1 << 33, 6, 7]
    p = device.puct_params(S, C_PUCT, 11, seed)  # 10 moves played < temp_plies
    moves, visits, q, trees = device.puct_search(states, gids, p, w, want_trees=True)
    for g in range(n):
        assert np.array_equal(visits[g], visits[0]) and visits[g].sum() == S
        pick = (rng.draw(rng.stream_key(seed, gids[g], 10, 0), 0) * S) >> 64
        run = np.cumsum(visits[g])
        assert int(moves[g]) == int(np.argmax(run > pick))
        assert trees[g]["main_draws"] == 1
    assert len(set(int(m) for m in moves)) > 1
    p0 = device.puct_params(S, C_PUCT, 0, seed)
    moves0, visits0, _, trees0 = device.puct_search(states, gids, p0, w, want_trees=True)
    assert np.array_equal(visits0, visits)
    for g in range(n):
        assert int(moves0[g]) == int(np.argmax(visits0[g])) and trees0[g]["main_draws"] == 0
    # temp_plies == the move count: no sampling either
    p1 = device.puct_params(S, C_PUCT, 10, seed)
    assert np.array_equal(device.puct_search(states, gids, p1, w)[0], moves0)


def test_ai_agent_puct_mode():
    from ai_agent import AIFactory
    from gomoku_board import GomokuBoard
    ai = AIFactory.create_ai("alphazero", 1, "easy", search="puct", seed=5, game_id=2)
    b0, b1 = GomokuBoard(), GomokuBoard()
    for r, c in ((7, 7), (7, 8), (8, 8)):
        b1.make_move(r, c)
    got = ai.get_moves([b0, b1], [2, 9])
    S = ai.params["num_simulations"]
    assert ai.last_search_visits.shape == (2, 225) and list(ai.last_search_visits.sum(axis=1)) == [S, S]
    assert ai.last_root_value.shape == (2,) and np.all(np.abs(ai.last_root_value) <= 1.0)
    p = device.puct_params(S, ai.params["c_puct"], 0, 5)
    states = np.concatenate([b0.to_state(), b1.to_state()])
    mv, visits, q, _ = device.puct_search(states, [2, 9], p, ai.model.device_weights())
    assert got == [(int(m) // 15, int(m) % 15) for m in mv]
    assert np.array_equal(visits, ai.last_search_visits) and np.array_equal(q, ai.last_root_value)
    assert b1.is_valid_move(*got[1]) and ai.get_move(b0) == got[0]  # no opening book: the search decides
    over = GomokuBoard()
    over.game_over = True
    assert ai.get_moves([over], [0]) == [None]


# ---------------------------------------------------------------- 4. self-play
def _replay(moves):
    """Play row-major moves from the empty board; returns (cells per ply, winner or 0, over)."""
    cells = [0] * 225
    before = []
    over, winner = False, 0
    for k, m in enumerate(moves):
        assert not over and cells[m] == 0, "illegal move in a record"
        before.append(tuple(cells))
        pl = 1 + k % 2
        cells[m] = pl
        if R.makes_five(cells, m, pl):
            over, winner = True, pl
        elif 0 not in cells or k + 1 >= 200:
            over = True
    return before, winner, over


def test_selfplay_puct():
    w = _weights("f16x3")
    S, n_slots, temp, seed = 16, 8, 6, 21
    eng = SelfPlayEngine(n_slots=n_slots, num_simulations=S, c_puct=C_PUCT, seed=seed, pv_weights=w,
                         search="puct", temp_plies=temp)
    # a default-mode engine alongside plays the golden games as before
    ref_eng = SelfPlayEngine(n_slots=6, num_simulations=2, c_puct=1.6, exploration=0.05, beta=0.0, seed=SEED,
                             plies_per_step=50, game_id_base=100, game_id_stride=6)
    with pytest.raises(ValueError):
        eng.compact()
    with pytest.raises(ValueError):
        ref_eng.visits()
    recs, vis, ref_recs = [], [], []
    steps = 0
    done = set()
    while steps < 600 and not (len(done) >= 8 and {0, 1} <= done):
        eng.step()
        steps += 1
        c = eng.counters()
        assert c["records_dropped"] == 0 and c["moves"] == n_slots and c["leaves"] == 0
        if c["records"]:
            r, v = eng.records(), eng.visits()
            assert len(r) == len(v) == c["records"]
            recs.append(r.copy())
            vis.append(v.copy())
            done |= set(int(x) for x in r["game_id"])
        if steps <= 2:
            ref_eng.step(50)
            ref_recs.append(ref_eng.records().copy())
    assert len(done) >= 8 and {0, 1} <= done, (steps, sorted(done))
    recs, vis = np.concatenate(recs), np.concatenate(vis)

    games = records_to_games(recs)
    total_plies = 0
    for gid, g in games.items():
        rows = vis[recs["game_id"] == gid][np.argsort(recs["ply"][recs["game_id"] == gid])]
        before, winner, over = _replay(g["moves"])
        assert over, gid
        total_plies += len(g["moves"])
        assert g["players"] == [1 + k % 2 for k in range(len(g["moves"]))]
        assert g["z"] == [0 if winner == 0 else (1 if pl == winner else -1) for pl in g["players"]]
        for k, m in enumerate(g["moves"]):
            assert tuple(int(x) for x in g["cells"][k]) == before[k]
            assert int(rows[k].sum()) == S
            assert not rows[k][np.array(before[k]) != 0].any()
            assert rows[k][m] > 0
            if k >= temp:
                assert m == int(np.argmax(rows[k]))

    # games 0 and 1 driven ply by ply from Python through gz_puct_search
    p = device.puct_params(S, C_PUCT, temp, seed)
    rows = {gid: vis[recs["game_id"] == gid][np.argsort(recs["ply"][recs["game_id"] == gid])] for gid in (0, 1)}
    cells = {gid: np.zeros(225, np.int8) for gid in (0, 1)}
    for k in range(max(len(games[0]["moves"]), len(games[1]["moves"]))):
        live = [gid for gid in (0, 1) if k < len(games[gid]["moves"])]
        states = np.concatenate([_state(cells[gid], k, 1 + k % 2) for gid in live])
        mv, v, _, _ = device.puct_search(states, live, p, w)
        for i, gid in enumerate(live):
            m = games[gid]["moves"][k]
            assert int(mv[i]) == m, (gid, k)
            assert np.array_equal(v[i], rows[gid][k].astype(np.int32)), (gid, k)
            cells[gid][m] = 1 + k % 2

    # counters and slot statistics
    st, gids_now = eng.boards()
    d = eng.draws()
    for s in range(n_slots):
        mine = [g for gid, g in games.items() if gid % n_slots == s and gid < gids_now[s]]
        assert gids_now[s] == s + n_slots * len(mine)
        plies = sum(len(g["moves"]) for g in mine) + int(st["n_moves"][s])
        assert plies == steps
        sampled = sum(min(len(g["moves"]), temp) for g in mine) + min(int(st["n_moves"][s]), temp)
        assert d[s][1] == sampled and d[s][2] == 0
        assert plies <= d[s][0] <= plies * (S + 1)
    assert total_plies == len(recs)

    gold = {g["game_id"]: g for g in golden("games")["games"]}
    got = records_to_games(np.concatenate(ref_recs))
    for gid in range(100, 106, 2):
        assert got[gid]["moves"] == gold[gid]["moves"] and got[gid]["z"] == gold[gid]["outcomes"]
