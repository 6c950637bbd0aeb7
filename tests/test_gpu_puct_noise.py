"""The Dirichlet noise at the PUCT search root on the GPU (GZ_PUCT_ROOT_NOISE,
csrc/gz_dirichlet.h and csrc/gz_puct.hip) against the plain-Python restatement in
tests/puct_noise_ref.py, bit for bit: the sampler kernel, whole trees through the step
API with a synthetic evaluator, re-rooted trees, the self-play engines (lock-step and
with tree reuse) with real weights driven again through the step API, and the training
collection."""
import numpy as np
import pytest
import torch

import puct_noise_ref as NR
import puct_ref as R
import puct_reuse_ref as RR
from gzero import boards, device
from gzero.boards import RECORD_DTYPE
from gzero.selfplay import SelfPlayEngine, records_to_games
from test_gpu_puct import C_PUCT, _assert_tree, _clear, _pattern_cells, _state, _thinned, _weights, make_synth
from test_gpu_puct_reuse import _cells_of, _empty, _search_on

pytestmark = pytest.mark.gpu

SEED = 3
BIG = (1 << 40) + 3


def _params(S, alpha, eps, temp_plies=0, seed=SEED, precision="f16x3"):
    return device.puct_params(S, C_PUCT, temp_plies, seed, precision, dirichlet_alpha=alpha, noise_eps=eps)


def _assert_rows(gpu, ref):
    """_assert_tree and every prior row of an evaluated live node, float64 bit for bit."""
    _assert_tree(gpu, ref)
    for k, t in enumerate(ref.term):
        if t == 0 and ref.prior[k] is not None:
            assert [float(x) for x in gpu["prior"][k]] == list(ref.prior[k]), k


# ---------------------------------------------------------------- 1. the sampler kernel
def _noise_boards():
    edges = np.zeros(225, np.int8)
    edges[[63, 64, 127, 128, 191, 192, 224]] = [1, 2, 1, 2, 1, 2, 1]
    late = _thinned(199, 12)
    cells = [np.zeros(225, np.int8), _clear(_pattern_cells(), [113]), _pattern_cells(), edges, late]
    states = np.concatenate([_state(c) for c in cells])
    assert list(states["n_moves"]) == [0, 224, 225, 7, 199]
    return cells, states, [0, 1, 2, BIG, 4]


@pytest.mark.parametrize("alpha", [0.03, 0.3, 2.5])
def test_root_noise_kernel_equals_the_reference(alpha):
    cells, states, gids = _noise_boards()
    want = [NR.eta_row(SEED, gids[g], int(states["n_moves"][g]), [x == 0 for x in cells[g]], alpha) for g in range(5)]
    got = device.puct_root_noise(states, gids, SEED, alpha)  # n = 5
    for g in range(5):
        assert [float(x) for x in got[g]] == want[g], g  # float64, bit for bit
        one = device.puct_root_noise(states[g:g + 1], gids[g:g + 1], SEED, alpha)  # n = 1
        assert np.array_equal(one[0], got[g]), g
        # the host build of the same code
        assert np.array_equal(device.puct_root_noise_host(SEED, gids[g], int(states["n_moves"][g]), cells[g] == 0,
                                                          alpha), got[g]), g
    assert got[1][113] == 1.0 and got[1].sum() == 1.0
    assert not got[2].any()
    assert not got[3][[63, 64, 127, 128, 191, 192, 224]].any() and (got[3][[62, 65, 126, 129, 190, 193, 223]] > 0).all()
    assert abs(got[0].sum() - 1.0) < 1e-12 and (got[0] > 0).sum() >= (200 if alpha >= 0.3 else 100)


# ---------------------------------------------------------------- 2. step API vs the reference
def _run_steps(states, gids, p, evals):
    n, S = len(states), p.num_simulations
    st = device.PuctStepper(states, gids, p)
    for rnd in range(S + 1):
        if rnd:
            st.select()
        rows, active = st.leaves()
        cells = _cells_of(rows)
        prior = np.zeros((n, 225), np.float64)
        value = np.zeros(n, np.float32)
        for g in range(n):
            if active[g]:
                prior[g], value[g] = evals[g](cells[g], None)
        st.backup(prior, value)
    moves, visits, q = st.finish()
    return moves, visits, q, st.trees()


def _step_states():
    states = np.concatenate([_state(_thinned(41, 1)), _state(_thinned(30, 2)), _state(np.zeros(225, np.int8))])
    return states, [11, BIG, 13], [make_synth(), make_synth(boost=[224]), make_synth()]


@pytest.mark.parametrize("eps", [0.25, 1.0])
@pytest.mark.parametrize("S", [1, 2, 120])
def test_step_api_trees_equal_the_reference(S, eps):
    alpha = 0.3
    states, gids, evals = _step_states()
    moves, visits, q, trees = _run_steps(states, gids, _params(S, alpha, eps), evals)
    for g, s in enumerate(states):
        cells = [int(x) for x in boards.words_to_cells(s["black"], s["white"])]
        noise = NR.Noise(SEED, gids[g], alpha, eps)
        ref = NR.search(cells, int(s["player"]), int(s["n_moves"]), S, C_PUCT, evals[g], noise)
        _assert_rows(trees[g], ref)
        assert list(visits[g]) == ref.root_visits() and int(visits[g].sum()) == S
        assert int(moves[g]) == R.choose_move(ref, 0, SEED, gids[g])[0]
        assert float(q[g]) == R.root_q(ref)
        # the root's row is the evaluator's mixed with eta, every other row the evaluator's own
        raw = evals[g](tuple(cells), None)[0]
        assert list(ref.prior[0]) != raw
        eta = NR.eta(SEED, gids[g], int(s["n_moves"]), [x == 0 for x in cells], alpha)
        if eps == 1.0:  # 0.0 * prior + 1.0 * eta: the row is eta itself at the empty cells
            assert [float(x) for x, c in zip(trees[g]["prior"][0], cells) if c == 0] == \
                [e for e, c in zip(eta, cells) if c == 0]
        for k in range(1, trees[g]["n_nodes"]):
            if trees[g]["term"][k] == 0:
                kc = tuple(int(x) for x in _cells_of(trees[g]["board"][k:k + 1])[0])
                assert [float(x) for x in trees[g]["prior"][k]] == evals[g](kc, None)[0], (g, k)


def test_eps_zero_is_the_flag_clear_tree():
    S = 24
    states, gids, evals = _step_states()
    plain = _run_steps(states, gids, device.puct_params(S, C_PUCT, 0, SEED), evals)
    zero = _run_steps(states, gids, _params(S, 0.3, 0.0), evals)
    for a, b in zip(plain[:3], zero[:3]):
        assert np.array_equal(a, b)
    for ta, tb in zip(plain[3], zero[3]):
        for key in ta:
            assert np.asarray(ta[key]).tobytes() == np.asarray(tb[key]).tobytes(), key


# ---------------------------------------------------------------- 3. re-root
def test_reroot_mixes_each_root_once():
    S, alpha, eps, n = 24, 0.3, 0.25, 3
    gids = [0, 1, BIG]
    evalf = make_synth()
    evals = [evalf] * n
    st = device.PuctStepper(_empty(n), gids, _params(S, alpha, eps))
    noises = [NR.Noise(SEED, g, alpha, eps) for g in gids]
    refs = [RR.fresh([0] * 225, 1, 0) for _ in range(n)]
    remaining = np.full(n, S + 1)
    for ply in range(3):
        for ref, noise in zip(refs, noises):  # roots that wait for their evaluation: mixed at that backup
            if ref.prior[0] is None:
                NR.evaluate(ref, evalf, noise)
        _search_on(st, evals, remaining)
        moves, visits, _ = st.finish()
        before = st.trees()
        for g, ref in enumerate(refs):
            while ref.visits[0] < S + 1:
                RR.simulate(ref, C_PUCT, evalf)
            _assert_rows(before[g], ref)
            assert list(visits[g]) == ref.root_visits() and int(visits[g].sum()) == S
            assert int(moves[g]) == R.choose_move(ref, 0, SEED, gids[g])[0]
        # game 0 follows its search; game 1 stays where it is on the first ply; game 2 plays a
        # cell its search never tried on the second
        play = [int(m) for m in moves]
        if ply == 0:
            play[1] = -1
        if ply == 1:
            play[2] = next(c for c in range(225) if refs[2].cells[0][c] == 0 and c not in refs[2].child[0])
        carried = [None if m < 0 or m not in ref.child[0] else list(ref.prior[ref.child[0][m]])
                   for m, ref in zip(play, refs)]
        remaining = st.reroot(play)
        rows, active = st.leaves()
        after = st.trees()
        for g, m in enumerate(play):
            if m < 0:  # the tree is untouched: no second mix of its root
                for key in before[g]:
                    assert np.array_equal(before[g][key], after[g][key]), key
                assert remaining[g] == 0 and not active[g]
                continue
            refs[g], over = NR.advance(refs[g], m, noises[g])
            assert not over
            assert int(remaining[g]) == S + 1 - refs[g].visits[0]
            if carried[g] is None:  # a fresh root: nothing stored yet, its board is the leaf
                assert active[g] and after[g]["n_nodes"] == 1 and after[g]["n_evals"] == 0
                assert refs[g].prior[0] is None and list(after[g]["visits"]) == [0]
                assert tuple(int(x) for x in _cells_of(rows)[g]) == refs[g].cells[0]
            else:  # an inherited root: its carried row mixed once with the new ply's eta
                assert not active[g]
                _assert_rows(after[g], refs[g])
                want = NR.mix(carried[g], refs[g].cells[0], SEED, gids[g], refs[g].count[0], alpha, eps)
                assert [float(x) for x in after[g]["prior"][0]] == want and want != carried[g]
                assert evalf(refs[g].cells[0], None)[0] == carried[g]
    assert [r.count[0] for r in refs] == [3, 2, 3]


# ---------------------------------------------------------------- 4. the engines, real weights
ENG = dict(S=16, seed=21, alpha=0.3, eps=0.25, games=6)
_PLAYED = {}


def _play(n_slots, reuse, alpha):
    """Games 0..5 at temp_plies 0 -> (records sorted by (id, ply), their visit rows)."""
    key = (n_slots, reuse, alpha)
    if key not in _PLAYED:
        S, n_games = ENG["S"], ENG["games"]
        eng = SelfPlayEngine(n_slots=n_slots, num_simulations=S, c_puct=C_PUCT, seed=ENG["seed"],
                             pv_weights=_weights("f16x3"), search="puct", temp_plies=0, tree_reuse=reuse,
                             game_id_end=n_games if reuse else None, dirichlet_alpha=alpha, noise_eps=ENG["eps"])
        recs, vis, done = [], [], set()
        for _ in range(-(-n_games // n_slots) * 200 + 2):
            eng.step()
            c = eng.counters()
            assert c["records_dropped"] == 0
            if c["records"]:
                r, v = eng.records().copy(), eng.visits().copy()
                keep = r["game_id"] < n_games
                recs.append(r[keep])
                vis.append(v[keep])
                done |= set(int(x) for x in r["game_id"][keep])
            if len(done) == n_games:
                break
        assert len(done) == n_games
        recs, vis = np.concatenate(recs), np.concatenate(vis)
        order = np.lexsort((recs["ply"], recs["game_id"]))
        _PLAYED[key] = (recs[order], vis[order])
    return _PLAYED[key]


def _root_rows_are_mixed_forwards(trees, gids, plies):
    """Every live root's stored row = the standalone forward of its board mixed with the
    reference's eta of (game, ply)."""
    w = _weights("f16x3")
    rows = np.stack([t["board"][0] for t in trees])
    _, _, _, fprior = device.pv_forward(w, rows, want_prior=True)
    cells = _cells_of(rows)
    for g, t in enumerate(trees):
        if t["term"][0] == 0 and t["n_evals"] > 0:
            want = NR.mix([float(x) for x in fprior[g]], [int(x) for x in cells[g]], ENG["seed"], gids[g], plies[g],
                          ENG["alpha"], ENG["eps"])
            assert [float(x) for x in t["prior"][0]] == want, g


def _forward_backup(st, w, d_probs, d_prior):
    _, d_value, _ = device.pv_forward_dev(w, st.d_leaves, st.n, d_probs=d_probs, d_prior=d_prior)
    st.backup(d_prior, d_value)


@pytest.mark.parametrize("reuse", [False, True])
def test_engine_games_equal_the_step_api_replay(reuse):
    S, n, plies = ENG["S"], ENG["games"], 3
    recs, vis = _play(6, reuse, ENG["alpha"])
    assert (vis.astype(np.int64).sum(axis=1) == S).all()
    games = records_to_games(recs)
    assert sorted(games) == list(range(n)) and all(len(g["moves"]) >= plies for g in games.values())
    w = _weights("f16x3")
    p = _params(S, ENG["alpha"], ENG["eps"], 0, ENG["seed"])
    gids = list(range(n))
    d_probs = torch.empty(n * 225, dtype=torch.float32, device="cuda")
    d_prior = torch.empty(n * 225, dtype=torch.float64, device="cuda")
    cells = np.zeros((n, 225), np.int8)
    st, remaining = None, S
    for ply in range(plies):
        if st is None or not reuse:  # lock-step: a fresh search of every position
            st = device.PuctStepper(np.concatenate([_state(c, ply, 1 + ply % 2) for c in cells]), gids, p)
            _forward_backup(st, w, d_probs, d_prior)
            remaining = S
        for _ in range(int(remaining)):
            st.select()
            _forward_backup(st, w, d_probs, d_prior)
        moves, visits, _ = st.finish()
        _root_rows_are_mixed_forwards(st.trees(), gids, [ply] * n)
        for g in range(n):
            assert int(moves[g]) == games[g]["moves"][ply], (g, ply)
            assert np.array_equal(visits[g], vis[recs["game_id"] == g][ply].astype(np.int32)), (g, ply)
            cells[g][int(moves[g])] = 1 + ply % 2
        if reuse:
            rem = st.reroot(moves)
            assert not st.d_active.cpu().numpy().any()  # the move played is the most visited: it has a child
            _root_rows_are_mixed_forwards(st.trees(), gids, [ply + 1] * n)
            remaining = int(rem.max())  # (a game at its budget has an inactive row until the last is done)


@pytest.mark.parametrize("reuse", [False, True])
def test_games_do_not_depend_on_the_slot_count(reuse):
    a = _play(6, reuse, ENG["alpha"])
    b = _play(3, reuse, ENG["alpha"])
    assert len(a[0]) == len(b[0]) and a[0].tobytes() == b[0].tobytes()
    assert np.array_equal(a[1], b[1])


@pytest.mark.parametrize("reuse", [False, True])
def test_noise_makes_the_games_differ(reuse):
    off = records_to_games(_play(6, reuse, None)[0])
    on = records_to_games(_play(6, reuse, ENG["alpha"])[0])
    # temp_plies 0: without noise every game is the same deterministic line of play
    assert all(off[g]["moves"] == off[0]["moves"] for g in range(ENG["games"]))
    lines = {tuple(on[g]["moves"]) for g in range(ENG["games"])}
    print(f"reuse={reuse}: {len(lines)} distinct games of 6 with noise, 1 without")
    assert len(lines) >= 2


# ---------------------------------------------------------------- 5. training
def test_training_collection_with_noise():
    import training
    from gzero.train import DeviceTrainer
    from test_gpu_puct_train import _model
    S, n_games, base, seed = 8, 4, 12, 11
    model = _model()
    DeviceTrainer(model)
    kw = dict(num_simulations=S, seed=seed, game_id_base=base, model=model, temp_plies=0)
    d, d_vis, n, st = training.selfplay_puct_device(n_games, dirichlet_alpha=0.3, **kw)
    recs = np.frombuffer(d.cpu().numpy().tobytes(), RECORD_DTYPE)
    vis = d_vis.cpu().numpy().view(np.uint16)
    assert len(recs) == len(vis) == n and st["games"] == n_games
    assert sorted(set(int(g) for g in recs["game_id"])) == list(range(base, base + n_games))
    assert (vis.astype(np.int64).sum(axis=1) == S).all()
    # None plays the noise-free games, byte for byte the call without the argument
    d0, v0, n0, _ = training.selfplay_puct_device(n_games, **kw)
    d1, v1, n1, _ = training.selfplay_puct_device(n_games, dirichlet_alpha=None, noise_eps=0.5, **kw)
    assert n0 == n1 and d0.cpu().numpy().tobytes() == d1.cpu().numpy().tobytes()
    assert v0.cpu().numpy().tobytes() == v1.cpu().numpy().tobytes()
    assert d.cpu().numpy().tobytes() != d0.cpu().numpy().tobytes()
