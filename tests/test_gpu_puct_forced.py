"""Forced playouts and policy-target pruning on the GPU (GZ_PUCT_FORCED_PLAYOUTS:
csrc/gz_forced.h, csrc/gz_puct.hip) against the plain-Python restatement in
tests/puct_forced_ref.py: the step API round by round on a synthetic evaluator,
gz_puct_search with the real forward and root noise, the lock-step and the own-clock
self-play engines (with the playout cap, slot counts, round cuts, compaction and leaf
symmetry), neutrality of the flag when clear and at k = 0, the argument errors, and the
pruned rows as training targets.

Every bit-for-bit case also asserts, from the reference's own counters, that the search it
compares forced at least one selection and pruned at least one visit: a case in which
nothing was forced would pass on an engine that ignores the flag."""
import ctypes

import numpy as np
import pytest
import torch

import puct_forced_ref as FR
import puct_noise_ref as NR
import puct_ref as R
import puct_sym_ref as SR
from gzero import _lib, boards, device
from gzero.selfplay import SelfPlayEngine, records_to_games
from test_gpu_puct import C_PUCT, _assert_tree, _five_states, _state, _weights
from test_puct_forced_cpu import X, Y, peaked_eval  # noqa: F401

pytestmark = pytest.mark.gpu

K = 2.0
ALPHA, EPS = 0.3, 0.25
_CACHE = {}


def _assert_tree_and_priors(gpu, ref):
    _assert_tree(gpu, ref)
    for k, t in enumerate(ref.term):
        if t == 0 and ref.prior[k] is not None:
            assert [float(x) for x in gpu["prior"][k]] == list(ref.prior[k]), k  # float64, bit for bit


# ---------------------------------------------------------------- 1. step API, synthetic evaluator
def _synth(cells, player=None):
    """peaked_eval with the side to move taken from the stone count (the step API's
    caller sees boards only)."""
    cells = tuple(int(x) for x in cells)
    return peaked_eval(cells, 1 + sum(1 for x in cells if x) % 2)


def _step_states():
    """4 games: the empty board, and three with stones away from X and Y (even counts:
    black to move), so the four trees differ."""
    out = [np.zeros(225, np.int8)]
    for g in range(1, 4):
        c = np.zeros(225, np.int8)
        for i in range(2 * g):
            c[3 + 17 * i + g] = 1 + i % 2
        assert c[X] == 0 and c[Y] == 0
        out.append(c)
    return out


def test_step_api_equals_the_reference_round_by_round():
    S, n, seed = 40, 4, 3
    cells = _step_states()
    states = np.concatenate([_state(c) for c in cells])
    gids = [10, 11, 12, 13]
    p = device.puct_params(S, C_PUCT, 0, seed, forced_playouts=K)
    st = device.PuctStepper(states, gids, p)
    refs = [None] * n
    cnt = [FR.Counters() for _ in range(n)]
    for rnd in range(S + 1):
        if rnd:
            st.select()
        rows, active = st.leaves()
        leaf = boards.words_to_cells(rows[:, :8], rows[:, 8:])
        prior = np.zeros((n, 225), np.float64)
        value = np.zeros(n, np.float32)
        for g in range(n):
            if active[g]:
                prior[g], value[g] = _synth(leaf[g])
        st.backup(prior, value)
        trees = st.trees()
        for g in range(n):
            if rnd == 0:
                refs[g] = FR.RR.fresh([int(x) for x in cells[g]], int(states[g]["player"]), int(states[g]["n_moves"]),
                                      _synth)
            else:
                FR.simulate(refs[g], C_PUCT, _synth, K, cnt[g])
            _assert_tree_and_priors(trees[g], refs[g])
    moves, visits, q = st.finish()
    after = st.trees()
    for g in range(n):
        raw = refs[g].root_visits()
        want = FR.prune_row(refs[g], C_PUCT, K, cnt[g])
        assert [int(x) for x in visits[g]] == want, g
        assert int(moves[g]) == R.choose_move(refs[g], 0, seed, gids[g])[0]
        assert float(q[g]) == R.root_q(refs[g])
        _assert_tree_and_priors(after[g], refs[g])  # the tree keeps the raw counts
        assert cnt[g].forced_selections >= 1 and cnt[g].pruned_visits >= 1, g
        assert raw[X] > want[X] and sum(want) < S == sum(raw)


# ---------------------------------------------------------------- 2. gz_puct_search, real forward, noise
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_search_with_real_weights_and_noise(precision):
    w = _weights(precision)
    S, seed = 64, 9
    states = np.concatenate([_five_states(), _state(np.zeros(225, np.int8))])
    n, gids = len(states), [20, 21, 22, 23, 24, (1 << 40) + 5]
    p = device.puct_params(S, C_PUCT, 0, seed, precision, dirichlet_alpha=ALPHA, noise_eps=EPS, forced_playouts=K)
    moves, visits, q, trees = device.puct_search(states, gids, p, w, want_trees=True)
    _, _, _, raw_prior = device.pv_forward(w, np.stack([t["board"][0] for t in trees]), want_prior=True)
    for g in range(n):
        t = trees[g]
        cells = boards.words_to_cells(t["board"][:, :8], t["board"][:, 8:])
        s = states[g]
        # the root row is the forward's row mixed with the reference's noise of (game, ply) ...
        want_root = NR.mix([float(x) for x in raw_prior[g]], [int(x) for x in cells[0]], seed, gids[g],
                           int(s["n_moves"]), ALPHA, EPS)
        assert [float(x) for x in t["prior"][0]] == want_root, g
        # ... and the reference driven with the GPU's own evaluations (the root's already mixed)
        table = {tuple(int(x) for x in cells[k]): ([float(x) for x in t["prior"][k]], float(t["value"][k]))
                 for k in range(t["n_nodes"]) if t["term"][k] == 0}

        def evalf(c, player, table=table):
            assert tuple(c) in table, "the reference asks for a board the GPU tree lacks"
            return table[tuple(c)]

        cnt = FR.Counters()
        ref = FR.search([int(x) for x in cells[0]], int(s["player"]), int(s["n_moves"]), S, C_PUCT, evalf, K,
                        counters=cnt)
        _assert_tree_and_priors(t, ref)
        assert [int(x) for x in visits[g]] == FR.prune_row(ref, C_PUCT, K, cnt), g
        assert int(moves[g]) == R.choose_move(ref, 0, seed, gids[g])[0]
        assert float(q[g]) == R.root_q(ref)
        assert 0 < visits[g].sum() <= S
        print(f"{precision} game {g}: forced selections {cnt.forced_selections}, pruned {cnt.pruned_visits}")
        # the condition of the case, per game: the reference itself forced and pruned
        assert cnt.forced_selections >= 1 and cnt.pruned_visits >= 1, g


# ---------------------------------------------------------------- 3. the engines
S_ENG, TEMP, SEED, GAMES, REF_PLIES = 48, 2, 7, 6, 6
FAST, PROB = 8, 0.5


POLICY_SCALE = 128.0


def _eng_weights():
    """The init weights with the policy FC scaled by 128, as tests/test_gpu_puct_cap.py: under
    the init weights' nearly flat prior a 48-simulation root has no child that stands out, the
    forced visits of a noised cell are then earned by PUCT's own arithmetic and nothing is
    pruned; with a favourite child they are not."""
    if "w" not in _CACHE:
        from gzero import weights
        sd = weights.init_state_dict(0)
        sd["policy_fc.weight"] = sd["policy_fc.weight"] * POLICY_SCALE
        sd["policy_fc.bias"] = sd["policy_fc.bias"] * POLICY_SCALE
        _CACHE["w"] = device.PVWeights(weights.pack_pv_weights(sd), "f16x3")
    return _CACHE["w"]


def _evalf(cells, player):
    """gz_pv_forward of the one board (a row's result does not depend on its batch), kept."""
    table = _CACHE.setdefault("evals", {})
    cells = tuple(int(x) for x in cells)
    if cells not in table:
        bl, wh = boards.cells_to_words(np.array(cells, np.int8)[None])
        _, v, _, prior = device.pv_forward(_eng_weights(), boards.leaf_words(bl, wh), want_prior=True)
        table[cells] = ([float(x) for x in prior[0]], float(v[0]))
    return table[cells]


def _play(n_slots, reuse, rounds_per_step=None, compact=False, **kw):
    """Games 0..5 -> (records sorted by (id, ply), their visit rows)."""
    key = ("play", n_slots, reuse, rounds_per_step, compact, tuple(sorted(kw.items())))
    if key not in _CACHE:
        eng = SelfPlayEngine(n_slots=n_slots, num_simulations=S_ENG, c_puct=C_PUCT, seed=SEED,
                             pv_weights=_eng_weights(), search="puct", temp_plies=TEMP, tree_reuse=reuse,
                             rounds_per_step=rounds_per_step, game_id_end=GAMES if (reuse or compact) else None,
                             compact_slots=compact, **kw)
        recs, vis, done = [], [], set()
        per_step = eng.rounds_per_step if reuse else S_ENG + 1
        for _ in range(-(-GAMES // n_slots) * 201 * (S_ENG + 1) // per_step + 2):
            eng.step()
            c = eng.counters()
            assert c["records_dropped"] == 0
            if c["records"]:
                r, v = eng.records().copy(), eng.visits().copy()
                keep = r["game_id"] < GAMES
                recs.append(r[keep])
                vis.append(v[keep])
                done |= set(int(x) for x in r["game_id"][keep])
            if len(done) == GAMES:
                break
            if compact:
                eng.n_active = int(eng.compact().item())
        assert len(done) == GAMES
        recs, vis = np.concatenate(recs), np.concatenate(vis)
        order = np.lexsort((recs["ply"], recs["game_id"]))
        _CACHE[key] = (recs[order], vis[order])
    return _CACHE[key]


def _reference(reuse, cap, sym):
    key = ("ref", reuse, cap, sym)
    if key not in _CACHE:
        out = []
        ev = SR.wrap(_evalf, SEED) if sym else _evalf
        for gid in range(GAMES):
            cnt = FR.Counters()
            moves, rows, raws, z, fulls = FR.play_game(
                SEED, gid, S_ENG, C_PUCT, TEMP, ev, K, noise=NR.Noise(SEED, gid, ALPHA, EPS), reuse=reuse,
                F=FAST if cap else None, full_prob=PROB, max_plies=REF_PLIES, counters=cnt)
            out.append(dict(moves=moves, rows=rows, raws=raws, fulls=fulls, cnt=cnt))
        _CACHE[key] = out
    return _CACHE[key]


def _compare(played, ref, cap):
    recs, vis = played
    games = records_to_games(recs)
    assert sorted(games) == list(range(GAMES))
    fast_seen = 0
    for gid, r in enumerate(ref):
        k = len(r["moves"])
        assert k == REF_PLIES or len(games[gid]["moves"]) == k
        assert games[gid]["moves"][:k] == r["moves"], gid
        rows = vis[recs["game_id"] == gid][:k].astype(np.int32)
        assert [list(map(int, x)) for x in rows] == r["rows"], gid
        for ply in range(k):
            if not r["fulls"][ply]:  # a fast ply is neither forced nor pruned
                assert r["rows"][ply] == r["raws"][ply]
                fast_seen += 1
        print(f"game {gid}: forced selections {r['cnt'].forced_selections}, pruned visits {r['cnt'].pruned_visits}")
    # the condition of the case, per game: the reference itself forced and pruned in the plies compared
    for gid, r in enumerate(ref):
        assert r["cnt"].forced_selections >= 1 and r["cnt"].pruned_visits >= 1, gid
    assert any(r["rows"] != r["raws"] for r in ref)
    assert (fast_seen >= 1) == cap


FORCED = dict(dirichlet_alpha=ALPHA, noise_eps=EPS, forced_playouts=K)
CAP = dict(fast_simulations=FAST, full_prob=PROB)


def test_lock_step_engine_equals_the_reference():
    _compare(_play(6, False, **FORCED), _reference(False, False, False), False)


def test_lock_step_engine_with_leaf_symmetry_equals_the_reference():
    played = _play(6, False, leaf_symmetry=True, **FORCED)
    _compare(played, _reference(False, False, True), False)
    assert played[0].tobytes() != _play(6, False, **FORCED)[0].tobytes()


@pytest.mark.parametrize("compact", [False, True])
def test_own_clock_engine_equals_the_reference_whatever_the_slots(compact):
    a = _play(6, True, 17, **FORCED, **CAP)
    _compare(a, _reference(True, True, False), True)
    b = _play(3, True, 5, compact, **FORCED, **CAP)  # three slots: games 3, 4, 5 are refills
    assert len(a[0]) == len(b[0]) and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    if compact:
        c = _play(6, True, 17, True, **FORCED, **CAP)
        assert a[0].tobytes() == c[0].tobytes() and np.array_equal(a[1], c[1])
    # pruned rows only on full plies; every row still has a count to normalise by
    sums = a[1].astype(np.int64).sum(axis=1)
    assert (sums > 0).all() and (sums < S_ENG).any()


# ---------------------------------------------------------------- 4. flag neutrality
@pytest.mark.parametrize("reuse", [False, True])
def test_flag_clear_and_k_zero_give_the_engines_bytes(reuse):
    noise = dict(dirichlet_alpha=ALPHA, noise_eps=EPS)
    a = _play(6, reuse, **noise)
    b = _play(6, reuse, forced_playouts=0.0, **noise)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    assert (a[1].astype(np.int64).sum(axis=1) == S_ENG).all()
    c = _play(6, reuse, **FORCED)
    assert not np.array_equal(a[1][:len(c[1])], c[1][:len(a[1])])  # (k = 2 is not neutral)


def test_k_zero_trees_are_the_flag_clear_trees():
    w = _weights("f16x3")
    states, gids = _five_states(), [20, 21, 22, 23, 24]
    kw = dict(dirichlet_alpha=ALPHA, noise_eps=EPS)
    a = device.puct_search(states, gids, device.puct_params(32, C_PUCT, 0, 9, **kw), w, want_trees=True)
    b = device.puct_search(states, gids, device.puct_params(32, C_PUCT, 0, 9, forced_playouts=0.0, **kw), w,
                           want_trees=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    for ta, tb in zip(a[3], b[3]):
        assert ta["n_nodes"] == tb["n_nodes"]
        for key in ("W", "visits", "value", "parent", "move_of", "term", "board", "prior"):
            assert np.asarray(ta[key]).tobytes() == np.asarray(tb[key]).tobytes(), key


# ---------------------------------------------------------------- 5. argument errors
def _forced_params(k, flags=0, S=8):
    return _lib.PuctForcedParams(S, 0, C_PUCT, 1, _lib.GZ_PV_F16X3, _lib.GZ_PUCT_FORCED_PLAYOUTS | flags, 0.3, 0.25, 4, 0,
                                 4, 0, 0.5, k)


def test_argument_errors_launch_nothing():
    L = _lib.load()
    n, S = 2, 8
    ws = torch.full((L.gz_selfplay_puct_workspace_bytes(n, S) + 4096,), 0x5A, dtype=torch.uint8, device="cuda")
    before = ws.clone()
    ptr = ctypes.c_void_p(ws.data_ptr())
    bad = [(_forced_params(float("nan")), b"forced_k"), (_forced_params(-1.0), b"forced_k"),
           (_forced_params(17.0), b"forced_k"), (_forced_params(2.0, _lib.GZ_PUCT_LEAF_BATCH), b"leaf batching")]
    for p, word in bad:
        pp = ctypes.cast(ctypes.pointer(p), ctypes.POINTER(_lib.PuctParams))
        calls = [
            lambda: L.gz_puct_begin(ptr, ptr, n, pp, ptr, ptr, ptr, None),
            lambda: L.gz_puct_search(ptr, ptr, n, pp, ptr, ptr, ptr, ptr, ptr, None),
            lambda: L.gz_selfplay_puct_run(ptr, n, pp, ptr, ptr, 1, ptr, 16, ptr, ptr, None),
            lambda: L.gz_selfplay_puct_run_active(ptr, n, n, pp, ptr, ptr, 1, ptr, 16, ptr, ptr, None),
            lambda: L.gz_selfplay_puct_rounds(ptr, n, pp, ptr, ptr, 1, ptr, 16, ptr, ptr, None),
            lambda: L.gz_selfplay_puct_rounds_active(ptr, n, n, pp, ptr, ptr, 1, ptr, 16, ptr, ptr, None),
        ]
        for call in calls:
            assert call() == -1 and word in L.gz_last_error(), L.gz_last_error()
    good = _forced_params(2.0)
    mp = _lib.PuctMatchParams(ctypes.cast(ctypes.pointer(good), ctypes.c_void_p), (ctypes.c_void_p * 2)(ptr, ptr),
                              (ctypes.c_int32 * 2)(_lib.GZ_PV_F16X3, _lib.GZ_PV_F16X3), 0, 0)
    assert L.gz_puct_match_run(ptr, n, n, ctypes.byref(mp), ptr, 1, ptr, 16, ptr, ptr, None) == -1
    assert b"forced playouts" in L.gz_last_error()
    torch.cuda.synchronize()
    assert torch.equal(ws, before)


# ---------------------------------------------------------------- 6. the pruned rows as targets
def test_pruned_rows_train():
    import pi_ref
    from gzero.train import DeviceDataset
    from test_gpu_pi import _pi, _same_bits
    recs, vis = _play(6, False, **FORCED)
    sums = vis.astype(np.int64).sum(axis=1)
    pick = np.flatnonzero(sums < S_ENG)[:12]
    assert len(pick) >= 4
    rows, rec = np.ascontiguousarray(vis[pick]), recs[pick].copy()
    n = len(rows)
    sel = list(range(n))  # every row under all 8 symmetries
    got = _pi(rows, sel, None)
    assert _same_bits(got, pi_ref.pi_dataset(rows, sel))
    base = rows.astype(np.float32) / rows.astype(np.int64).sum(axis=1).astype(np.float32)[:, None]
    assert _same_bits(got[:n], base)
    ds = DeviceDataset(rec, use_augmentation=False, visits=rows)
    assert ds.soft and _same_bits(ds.materialize()[1].cpu().numpy(), base)


def test_training_iteration_with_forced_playouts():
    import gzero.train as gtrain
    import training
    from test_gpu_puct_train import _model
    model = _model()
    trainer = gtrain.DeviceTrainer(model)
    out = training.run_iteration(model, trainer, 0, 8, num_simulations=32, seed=5, search="puct", forced_playouts=2.0,
                                 dirichlet_alpha=0.3, temp_plies=TEMP, verbose=False, epochs=1)
    assert not out.get("skipped") and np.isfinite(out["train_loss"]) and np.isfinite(out["val_loss"])
    with pytest.raises(ValueError, match="forced_playouts needs search='puct'"):
        training.run_iteration(model, trainer, 0, 8, num_simulations=32, seed=5, forced_playouts=2.0, verbose=False)
