"""PUCT tree reuse between plies on the GPU (csrc/gz_puct.hip: gz_puct_reroot,
gz_selfplay_puct_rounds) against the plain-Python restatement in
tests/puct_reuse_ref.py: re-rooted trees through the step API with a synthetic
evaluator, the re-root's edge cases, the self-play engine with real weights driven
again through the step API, independence of the slot count and the round cut, and the
training collection."""
import numpy as np
import pytest
import torch

import puct_ref as R
import puct_reuse_ref as RR
from gzero import boards, device
from gzero.boards import RECORD_DTYPE
from gzero.selfplay import SelfPlayEngine, records_to_games
from test_gpu_puct import C_PUCT, _assert_tree, _replay, _state, _thinned, _uniform, _weights, make_synth

pytestmark = pytest.mark.gpu

# the step-API scenario (tests/test_puct_reuse_cpu.py checks what its reference reuses)
STEP_SIMS = (1, 2, 16, 64)
STEP_GIDS = (0, 1)
STEP_PLIES, STEP_TEMP, STEP_SEED = 12, 6, 3


# ---------------------------------------------------------------- drivers
def _cells_of(rows):
    return boards.words_to_cells(rows[:, :8], rows[:, 8:])


def _eval_round(st, evals):
    """Evaluate the current leaf rows on the host and back them up; returns active."""
    rows, active = st.leaves()
    cells = _cells_of(rows)
    prior = np.zeros((st.n, 225), np.float64)
    value = np.zeros(st.n, np.float32)
    for g in range(st.n):
        if active[g]:
            prior[g], value[g] = evals[g](cells[g], None)
        else:
            assert not rows[g].any(), "a game without a leaf leaves an empty board"
    st.backup(prior, value)
    return active


def _search_on(st, evals, remaining):
    """Run every game to its budget: `remaining` simulations left per game (a root that
    still waits for its evaluation counts as one of them)."""
    remaining = np.array(remaining)
    _, active = st.leaves()
    if active.any():  # roots waiting for their evaluation (after begin / a fresh root)
        remaining = remaining - _eval_round(st, evals)
    for rnd in range(int(remaining.max())):
        st.select()
        active = _eval_round(st, evals)
        assert not active[remaining <= rnd].any(), "a game at its budget has no leaf"


def _assert_tree_and_priors(gpu, ref):
    _assert_tree(gpu, ref)
    for k, t in enumerate(ref.term):
        if t == 0:
            assert [float(x) for x in gpu["prior"][k]] == list(ref.prior[k]), k  # float64, bit for bit


def _empty(n):
    return np.concatenate([_state(np.zeros(225, np.int8))] * n)


# ---------------------------------------------------------------- 1. step API vs the reference
@pytest.mark.parametrize("S", STEP_SIMS)
def test_step_api_reroot_equals_the_reference(S):
    evalf = make_synth()
    n = len(STEP_GIDS)
    evals = [evalf] * n
    p = device.puct_params(S, C_PUCT, STEP_TEMP, STEP_SEED)
    st = device.PuctStepper(_empty(n), STEP_GIDS, p)
    refs = [RR.fresh([0] * 225, 1, 0, evalf) for _ in range(n)]
    remaining = np.full(n, S + 1)
    kept = []
    for ply in range(STEP_PLIES):
        _search_on(st, evals, remaining)
        moves, visits, _ = st.finish()
        for g, (ref, tree) in enumerate(zip(refs, st.trees())):
            while ref.visits[0] < S + 1:
                RR.simulate(ref, C_PUCT, evalf)
            _assert_tree_and_priors(tree, ref)
            assert list(visits[g]) == ref.root_visits() and int(visits[g].sum()) == S
            assert int(moves[g]) == R.choose_move(ref, STEP_TEMP, STEP_SEED, STEP_GIDS[g])[0]
        remaining = st.reroot(moves)
        rows, active = st.leaves()
        assert not active.any() and not rows.any()
        for g, tree in enumerate(st.trees()):
            refs[g], over = RR.advance(refs[g], int(moves[g]))
            assert not over
            _assert_tree_and_priors(tree, refs[g])
            assert tree["move"] == -1 and tree["main_draws"] == 0
            assert int(remaining[g]) == S + 1 - refs[g].visits[0] >= 1
            kept.append((len(refs[g].parent), len({RR.depth_of(refs[g], k) for k in range(len(refs[g].parent))})))
    print(f"S={S}: kept (nodes, depths) per re-root {kept}")
    if S == 64:
        assert any(k >= 8 and d >= 3 for k, d in kept)
    if S == 1:
        assert all(k == 1 for k, d in kept)


# ---------------------------------------------------------------- 2. re-root edges
def test_reroot_edges():
    S = 120
    tcells, tplayer, tmoves = R.tactical_position()
    a, b = _thinned(41, 1), _thinned(30, 2)
    states = np.concatenate([_state(a), _state(b), _state(tcells, tmoves, tplayer)])
    evals = [make_synth(), make_synth(), _uniform]
    p = device.puct_params(S, C_PUCT, 0, 3)
    st = device.PuctStepper(states, [11, 12, 13], p)
    _search_on(st, evals, [S + 1] * 3)
    moves, visits, _ = st.finish()
    before = st.trees()
    refs = [R.search([int(x) for x in c], int(s["player"]), int(s["n_moves"]), S, C_PUCT, e)
            for c, s, e in zip((a, b, tcells), states, evals)]
    for t, ref in zip(before, refs):
        _assert_tree(t, ref)
    # game 0: an empty cell the search never tried; game 1: no move; game 2: black's five
    cold = next(c for c in range(225) if a[c] == 0 and visits[0][c] == 0)
    assert int(moves[2]) == 107 and refs[2].term[refs[2].child[0][107]] == 1
    remaining = st.reroot([cold, -1, 107])
    rows, active = st.leaves()
    after = st.trees()
    assert list(remaining) == [S + 1, 0, 0] and list(active) == [True, False, False]

    fresh, over = RR.advance(refs[0], cold)
    assert not over and len(fresh.parent) == 1
    assert tuple(int(x) for x in _cells_of(rows)[0]) == fresh.cells[0] and not rows[1:].any()
    t = after[0]
    assert t["n_nodes"] == 1 and t["n_evals"] == 0 and list(t["visits"]) == [0] and list(t["parent"]) == [-1]
    assert tuple(int(x) for x in _cells_of(t["board"])[0]) == fresh.cells[0]

    for key in before[1]:  # move -1: the tree is untouched
        assert np.array_equal(before[1][key], after[1][key]), key

    won, over = RR.advance(refs[2], 107)
    assert over and won.term == [1]
    _assert_tree(after[2], won)

    # the searches go on: the fresh root is a search of its own, the others have no leaf
    _search_on(st, evals, remaining)
    trees = st.trees()
    _assert_tree_and_priors(trees[0], R.search(list(fresh.cells[0]), fresh.player[0], fresh.count[0], S, C_PUCT,
                                               evals[0]))
    for g in (1, 2):
        for key in after[g]:
            assert np.array_equal(after[g][key], trees[g][key]), (g, key)
    m2, v2, _ = st.finish()
    assert int(m2[2]) == -1 and not v2[2].any()  # the game is over


def test_reroot_past_node_255():
    S = 300
    late = _thinned(185, 5)  # 40 empties
    evalf = make_synth()
    p = device.puct_params(S, C_PUCT, 0, 3)
    st = device.PuctStepper(_state(late), [5], p)
    _search_on(st, [evalf], [S + 1])
    moves, _, _ = st.finish()
    ref = R.search([int(x) for x in late], 2, 185, S, C_PUCT, evalf)
    j = ref.child[0][int(moves[0])]
    below = [k for k in range(len(ref.parent)) if _under(ref, k, j)]  # j and its descendants
    assert max(below) > 255 and len(below) > 20
    remaining = st.reroot(moves)
    nref, over = RR.advance(ref, int(moves[0]))
    assert not over and len(nref.parent) == len(below)
    _assert_tree_and_priors(st.trees()[0], nref)
    assert int(remaining[0]) == S + 1 - nref.visits[0]
    # and the next search, whose new nodes land above the kept ones
    _search_on(st, [evalf], remaining)
    while nref.visits[0] < S + 1:
        RR.simulate(nref, C_PUCT, evalf)
    assert len(nref.parent) > 256
    _assert_tree_and_priors(st.trees()[0], nref)


def _under(t, k, j):
    while k >= 0 and k != j:
        k = t.parent[k]
    return k == j


# ---------------------------------------------------------------- 3. the engine, real weights
ENG = dict(S=16, temp=6, seed=21)
_PLAYED = {}


def _play(precision, n_slots, rounds_per_step, n_games):
    """Games 0..n_games-1 on a reuse engine -> (records sorted by (id, ply), visit rows,
    per-slot statistics, rounds run)."""
    key = (precision, n_slots, rounds_per_step, n_games)
    if key not in _PLAYED:
        eng = SelfPlayEngine(n_slots=n_slots, num_simulations=ENG["S"], c_puct=C_PUCT, seed=ENG["seed"],
                             pv_weights=_weights(precision), search="puct", temp_plies=ENG["temp"], tree_reuse=True,
                             rounds_per_step=rounds_per_step, game_id_end=n_games)
        with pytest.raises(ValueError):
            eng.compact()
        recs, vis, done, steps = [], [], 0, 0
        max_steps = -(-n_games // n_slots) * 200 * (ENG["S"] + 1) // eng.rounds_per_step + 2
        while done < n_games and steps < max_steps:
            eng.step()
            steps += 1
            c = eng.counters()
            assert c["records_dropped"] == 0 and c["leaves"] == 0
            done += int(c["games"])
            if c["records"]:
                recs.append(eng.records().copy())
                vis.append(eng.visits().copy())
        assert done == n_games, (done, steps)
        recs, vis = np.concatenate(recs), np.concatenate(vis)
        order = np.lexsort((recs["ply"], recs["game_id"]))
        _PLAYED[key] = (recs[order], vis[order], eng.draws(), steps * eng.rounds_per_step)
    return _PLAYED[key]


def _drive_games(precision, gids, S, max_plies=200):
    """The same games through PuctStepper + reroot with gz_pv_forward as the evaluator:
    per game (moves, visit rows, evaluations per move, rounds per move)."""
    w = _weights(precision)
    n = len(gids)
    p = device.puct_params(S, C_PUCT, ENG["temp"], ENG["seed"], precision)
    st = device.PuctStepper(_empty(n), gids, p)
    d_probs = torch.empty(n * 225, dtype=torch.float32, device="cuda")
    d_prior = torch.empty(n * 225, dtype=torch.float64, device="cuda")
    out = [([], [], [], []) for _ in range(n)]
    evals = np.zeros(n, np.int64)

    def forward_backup():
        _, d_value, _ = device.pv_forward_dev(w, st.d_leaves, n, d_probs=d_probs, d_prior=d_prior)
        st.backup(d_prior, d_value)
        return st.d_active.cpu().numpy()

    evals += forward_backup()
    remaining = np.full(n, S)
    took = np.full(n, S + 1)
    checked = 0
    for ply in range(max_plies):
        for _ in range(int(remaining.max())):
            st.select()
            evals += forward_backup()
        moves, visits, _ = st.finish()
        if (moves < 0).all():
            break
        if ply % 8 == 0:  # stored priors and values = a standalone forward of the stored boards
            trees = st.trees()
            rows = np.concatenate([t["board"][t["term"] == 0] for t in trees])
            _, fv, _, fprior = device.pv_forward(w, rows, want_prior=True)
            assert np.array_equal(np.concatenate([t["prior"][t["term"] == 0] for t in trees]), fprior)
            assert np.array_equal(np.concatenate([t["value"][t["term"] == 0] for t in trees]), fv)
            checked += len(rows)
        for g in range(n):
            if moves[g] >= 0:
                out[g][0].append(int(moves[g]))
                out[g][1].append(visits[g].copy())
                out[g][2].append(int(evals[g]))
                out[g][3].append(int(took[g]))
                evals[g] = 0
        remaining = took = st.reroot(moves)
        assert not st.d_active.cpu().numpy().any()
    assert checked > 0
    return out


def test_selfplay_engine_with_tree_reuse():
    S, temp = ENG["S"], ENG["temp"]
    recs, vis, draws, rounds = _play("f16x3", 8, None, 8)
    games = records_to_games(recs)
    assert sorted(games) == list(range(8))
    total = 0
    for gid, g in games.items():
        rows = vis[recs["game_id"] == gid]
        before, winner, over = _replay(g["moves"])
        assert over, gid
        total += len(g["moves"])
        assert g["players"] == [1 + k % 2 for k in range(len(g["moves"]))]
        assert g["z"] == [0 if winner == 0 else (1 if pl == winner else -1) for pl in g["players"]]
        for k, m in enumerate(g["moves"]):
            assert tuple(int(x) for x in g["cells"][k]) == before[k]
            assert int(rows[k].sum()) == S
            assert not rows[k][np.array(before[k]) != 0].any()
            assert rows[k][m] > 0
            if k >= temp:
                assert m == int(np.argmax(rows[k]))
    assert total == len(recs)

    driven = _drive_games("f16x3", [0, 1], S)
    for gid, (moves, rows, evals, took) in zip((0, 1), driven):
        assert moves == games[gid]["moves"], gid
        assert np.array_equal(np.array(rows), vis[recs["game_id"] == gid].astype(np.int32)), gid
        # slot statistics: predicts = the rounds in which the slot's leaf was evaluated
        assert draws[gid][0] == sum(evals) < (S + 1) * len(moves), gid
        # ... main draws, and the rounds its moves took: S + 1 - the visits each root inherited
        assert draws[gid][1] == min(len(moves), temp)
        assert draws[gid][2] == sum(took) < (S + 1) * len(moves) and took[0] == S + 1
    rpm = sum(sum(t) for _, _, _, t in driven) / sum(len(m) for m, _, _, _ in driven)
    print(f"8 games, {total} plies, {rounds} rounds until the last ended; games 0 and 1: {rpm:.2f} rounds per move "
          f"(a fresh search per ply: {S + 1})")


def test_selfplay_engine_fp32_first_plies():
    """2 slots, S 4, the first 6 plies of each game round by round: the moves and the
    evaluations per move equal the step API's."""
    S, n, plies = 4, 2, 6
    w = _weights("fp32")
    eng = SelfPlayEngine(n_slots=n, num_simulations=S, c_puct=C_PUCT, seed=ENG["seed"], pv_weights=w, search="puct",
                         temp_plies=ENG["temp"], tree_reuse=True, rounds_per_step=1)
    driven = _drive_games("fp32", [0, 1], S, max_plies=plies)
    got = [([], [], []) for _ in range(n)]
    cells = np.zeros((n, 225), np.int8)
    seen = np.zeros((n, 3), np.int64)
    for rnd in range(plies * (S + 1) + 1):
        eng.step()
        st, gids = eng.boards()
        now = boards.words_to_cells(st["black"], st["white"])
        d = eng.draws()
        for s in range(n):
            if len(got[s][0]) < plies and int(st["n_moves"][s]) == len(got[s][0]) + 1 and gids[s] == s:
                (c,) = np.flatnonzero(now[s] != cells[s])
                got[s][0].append(int(c))
                got[s][1].append(int(d[s][0] - seen[s][0]))
                got[s][2].append(int(d[s][2] - seen[s][2]))
                seen[s] = d[s]
                cells[s] = now[s]
    for s in range(n):
        assert got[s][0] == driven[s][0][:plies] and len(got[s][0]) == plies, s
        assert got[s][1] == driven[s][2][:plies], s
        assert got[s][2] == driven[s][3][:plies], s


# ---------------------------------------------------------------- 4. independence
def test_games_do_not_depend_on_slots_or_round_cut():
    a = _play("f16x3", 6, 17, 6)
    b = _play("f16x3", 3, 5, 6)
    assert len(a[0]) == len(b[0]) and a[0].tobytes() == b[0].tobytes()
    assert np.array_equal(a[1], b[1])
    # and the eight-slot run of the engine test played the same six games
    recs, vis, _, _ = _play("f16x3", 8, None, 8)
    six = recs["game_id"] < 6
    assert recs[six].tobytes() == a[0].tobytes() and np.array_equal(vis[six], a[1])


# ---------------------------------------------------------------- 5. training
def test_training_collection_with_tree_reuse():
    import training
    from gzero.train import DeviceTrainer
    from test_gpu_puct_train import _model
    S, temp, n_games, base, seed = 8, 6, 4, 12, 11
    model = _model()
    DeviceTrainer(model)
    d, d_vis, n, st = training.selfplay_puct_device(n_games, num_simulations=S, seed=seed, game_id_base=base,
                                                    model=model, temp_plies=temp, tree_reuse=True)
    recs = np.frombuffer(d.cpu().numpy().tobytes(), RECORD_DTYPE)
    vis = d_vis.cpu().numpy().view(np.uint16)
    keys = [(int(g), int(p)) for g, p in zip(recs["game_id"], recs["ply"])]
    assert keys == sorted(keys) and len(set(keys)) == n and st["games"] == n_games
    assert sorted(set(int(g) for g in recs["game_id"])) == list(range(base, base + n_games))
    assert (vis.sum(axis=1) == S).all()
    # the same ids from an engine directly
    eng = SelfPlayEngine(n_slots=n_games, num_simulations=S, c_puct=1.6, seed=seed, pv_weights=model.device_weights(),
                         game_id_base=base, search="puct", temp_plies=temp, tree_reuse=True,
                         game_id_end=base + n_games)
    r2, v2, done = [], [], 0
    for _ in range(200):
        eng.step()
        c = eng.counters()
        done += int(c["games"])
        if c["records"]:
            r2.append(eng.records().copy())
            v2.append(eng.visits().copy())
        if done == n_games:
            break
    r2, v2 = np.concatenate(r2), np.concatenate(v2)
    order = np.lexsort((r2["ply"], r2["game_id"]))
    assert recs.tobytes() == r2[order].tobytes() and np.array_equal(vis, v2[order])
