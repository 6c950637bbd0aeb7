"""The Gumbel root with sequential halving on the GPU (GZ_PUCT_GUMBEL: csrc/gz_gumbel.h,
csrc/gz_puct.hip) against the plain-Python restatement in tests/puct_gumbel_ref.py: the step
API round by round on synthetic evaluators, gz_puct_search with the real forward against the
step API, the lock-step self-play engine (slot counts, compaction), the flag-clear bytes and
the untouched workspace tail, the argument errors, and the rows as training targets."""
import ctypes

import numpy as np
import pytest
import torch

import puct_gumbel_ref as GR
import puct_ref as R
from gzero import _lib, boards, device
from gzero.selfplay import SelfPlayEngine, records_to_games
from test_gpu_puct import C_PUCT, _assert_tree, _five_states, _state, _thinned, _weights, make_synth

pytestmark = pytest.mark.gpu

_CACHE = {}


def _assert_tree_and_priors(gpu, ref):
    _assert_tree(gpu, ref)
    for k, t in enumerate(ref.term):
        if t == 0 and ref.prior[k] is not None:
            assert [float(x) for x in gpu["prior"][k]] == list(ref.prior[k]), k  # float64, bit for bit


def _same_trees(a, b):
    for ta, tb in zip(a, b):
        assert ta["n_nodes"] == tb["n_nodes"] and ta["move"] == tb["move"] and ta["main_draws"] == tb["main_draws"]
        for key in ("W", "visits", "value", "parent", "move_of", "term", "board", "prior"):
            assert np.asarray(ta[key]).tobytes() == np.asarray(tb[key]).tobytes(), key


# ---------------------------------------------------------------- 1. step API, synthetic evaluators
def _uniform(cells, player=None):
    return R.uniform_eval([int(x) for x in cells], player)


_HASHED = make_synth()


def _hashed(cells, player=None):
    return _HASHED(cells, player)


def _step_states():
    """The empty board at ply 0, the tactical position (terminal children at the root) and a
    board with 3 empty cells at ply 150 (m becomes 3; the search reaches the full board)."""
    tcells, tplayer, tmoves = R.tactical_position()
    three = _thinned(222, 5)
    assert int((three == 0).sum()) == 3
    return [(np.zeros(225, np.int8), 0, 1), (np.array(tcells, np.int8), tmoves, tplayer), (three, 150, 1)]


@pytest.mark.parametrize("m,S", [(1, 5), (2, 5), (3, 7), (16, 16), (16, 33)])
@pytest.mark.parametrize("evalf", [_uniform, _hashed], ids=["uniform", "hashed"])
def test_step_api_equals_the_reference_round_by_round(evalf, m, S):
    seed, gids = 3, [10, 11, (1 << 40) + 12]
    pos = _step_states()
    n = len(pos)
    states = np.concatenate([_state(c, k, pl) for c, k, pl in pos])
    p = device.puct_params(S, C_PUCT, 4, seed, gumbel_considered=m)
    st = device.PuctStepper(states, gids, p)
    gms = [GR.Gumbel(seed, gid, m) for gid in gids]
    refs = [GR.new_tree([int(x) for x in c], pl, k) for c, k, pl in pos]
    waits = [0] * n
    idle = [0] * n
    for rnd in range(S + 1):
        if rnd:
            st.select()
            waits = [GR.select(refs[g], C_PUCT, GR.root_cell(refs[g], gms[g], S)) for g in range(n)]
        rows, active = st.leaves()
        leaf = boards.words_to_cells(rows[:, :8], rows[:, 8:])
        prior = np.zeros((n, 225), np.float64)
        value = np.zeros(n, np.float32)
        for g in range(n):
            assert bool(active[g]) == (waits[g] is not None), (rnd, g)
            idle[g] += waits[g] is None
            if active[g]:
                assert tuple(int(x) for x in leaf[g]) == refs[g].cells[waits[g]]
                prior[g], value[g] = evalf(leaf[g])
                GR.receive(refs[g], waits[g], [float(x) for x in prior[g]], float(value[g]), gms[g])
        st.backup(prior, value)
        trees = st.trees()
        for g in range(n):
            _assert_tree_and_priors(trees[g], refs[g])
    moves, rows, q = st.finish()
    after = st.trees()
    for g in range(n):
        ref, gm = refs[g], gms[g]
        v = ref.root_visits()
        assert sum(v) == S and len(ref.considered) == min(m, 3 if g == 2 else m)
        counts = sorted((v[c] for c in ref.considered), reverse=True)
        sched = GR.seq(len(ref.considered), S)
        assert counts[0] == sched[-1] + 1 and all(v[c] == 0 for c in range(225) if c not in ref.considered)
        assert int(moves[g]) == GR.choose_move(ref, gm), g
        pi, want = GR.target(ref, gm)
        assert [int(x) for x in rows[g]] == want, g
        assert float(q[g]) == R.root_q(ref)
        assert rows[g].max() >= 146 and not rows[g][np.array(ref.cells[0]) != 0].any()
        _assert_tree_and_priors(after[g], ref)  # the tree keeps the raw visits and the stored row
        assert after[g]["main_draws"] == 0 and after[g]["move"] == int(moves[g])
    # the condition of the case: on the nearly full board the searches of 16 and more simulations
    # ran into terminal nodes (rounds without a leaf)
    assert S < 16 or idle[2] >= 1


def test_reroot_on_a_gumbel_workspace_is_an_argument_error():
    states = _state(np.zeros(225, np.int8))
    st = device.PuctStepper(states, [1], device.puct_params(5, C_PUCT, 0, 3, gumbel_considered=2))
    st.backup(*[np.asarray(x) for x in (_uniform(np.zeros(225, np.int8))[0], [0.0])])
    before = st.ws.clone()
    with pytest.raises(Exception, match="tree reuse with the Gumbel root"):
        st.reroot([-1])
    torch.cuda.synchronize()
    assert torch.equal(st.ws, before)
    # a plain begin on the same workspace removes the note: the flag-clear kernels run again
    plain = device.puct_params(5, C_PUCT, 0, 3)
    d_states = device.to_dev(np.ascontiguousarray(states))
    d_gids = torch.as_tensor(np.asarray([1], np.int64)).cuda()
    _lib.check(st.lib.gz_puct_begin(device.ptr(d_states), device.ptr(d_gids), 1, ctypes.byref(plain), device.ptr(st.ws),
                                    device.ptr(st.d_leaves), device.ptr(st.d_active), device.stream()), "gz_puct_begin")
    st.backup(*[np.asarray(x) for x in (_uniform(np.zeros(225, np.int8))[0], [0.0])])
    assert st.reroot([-1])[0] == 5
    for _ in range(5):
        st.select()
        rows, active = st.leaves()
        leaf = boards.words_to_cells(rows[:, :8], rows[:, 8:])
        st.backup(np.asarray(_uniform(leaf[0])[0]), np.zeros(1, np.float32))
    moves, visits, _ = st.finish()
    ref = R.search([0] * 225, 1, 0, 5, C_PUCT, R.uniform_eval)
    assert [int(x) for x in visits[0]] == ref.root_visits() and int(moves[0]) == R.choose_move(ref, 0, 3, 1)[0]


# ---------------------------------------------------------------- 2. gz_puct_search, real forward
@pytest.mark.parametrize("sym", [False, True], ids=["plain", "leaf_sym"])
@pytest.mark.parametrize("precision", ["f16x3", "f16"])
def test_search_with_real_weights_equals_the_step_api(precision, sym):
    w = _weights(precision)
    S, seed = 16, 9
    states, gids = _five_states(), [20, 21, 22, 23, 24]
    p = device.puct_params(S, C_PUCT, 0, seed, precision, leaf_symmetry=sym, gumbel_considered=16)
    moves, rows, q, trees = device.puct_search(states, gids, p, w, want_trees=True)
    st = device.PuctStepper(states, gids, p)
    for rnd in range(S + 1):
        if rnd:
            st.select()
        st.backup(*st.evaluate(w))  # gz_pv_forward / gz_pv_forward_sym, standalone
    smoves, srows, sq = st.finish()
    assert np.array_equal(moves, smoves) and np.array_equal(rows, srows) and q.tobytes() == sq.tobytes()
    _same_trees(trees, st.trees())
    for g in range(len(gids)):
        if states[g]["over"]:
            continue
        assert rows[g].max() >= 146 and trees[g]["visits"][0] == S + 1 and trees[g]["main_draws"] == 0
        # the reference replayed with the tree's own evaluations reproduces search, move and row
        t = trees[g]
        cells = boards.words_to_cells(t["board"][:, :8], t["board"][:, 8:])
        table = {tuple(int(x) for x in cells[k]): ([float(x) for x in t["prior"][k]], float(t["value"][k]))
                 for k in range(t["n_nodes"]) if t["term"][k] == 0}
        gm = GR.Gumbel(seed, gids[g], 16)
        ref = GR.search([int(x) for x in cells[0]], int(states[g]["player"]), int(states[g]["n_moves"]), S, C_PUCT,
                        lambda c, pl, table=table: table[tuple(c)], gm)
        _assert_tree_and_priors(t, ref)
        assert int(moves[g]) == GR.choose_move(ref, gm) and [int(x) for x in rows[g]] == GR.target(ref, gm)[1]


# ---------------------------------------------------------------- 3. the lock-step engine
S_ENG, M_ENG, SEED, GAMES = 8, 4, 7, 6


def _eng_weights():
    return _weights("f16x3")


def _eval_batch(boards_cells):
    """gz_pv_forward of the boards in one launch (a row's result does not depend on its batch)."""
    bl, wh = boards.cells_to_words(np.array(boards_cells, np.int8))
    _, v, _, prior = device.pv_forward(_eng_weights(), boards.leaf_words(bl, wh), want_prior=True)
    return prior, v


def _reference_games():
    """Games 0..5 of the restatement, played in lock-step so that every round is one forward."""
    if "ref" in _CACHE:
        return _CACHE["ref"]
    games = {gid: dict(cells=[0] * 225, player=1, n=0, moves=[], rows=[], winner=None) for gid in range(GAMES)}
    gms = {gid: GR.Gumbel(SEED, gid, M_ENG) for gid in range(GAMES)}
    while True:
        live = [gid for gid, g in games.items() if g["winner"] is None]
        if not live:
            break
        trees = {gid: GR.new_tree(games[gid]["cells"], games[gid]["player"], games[gid]["n"]) for gid in live}
        waits = {gid: 0 for gid in live}
        for rnd in range(S_ENG + 1):
            if rnd:
                waits = {gid: GR.select(trees[gid], C_PUCT, GR.root_cell(trees[gid], gms[gid], S_ENG)) for gid in live}
            ask = [gid for gid in live if waits[gid] is not None]
            if ask:
                prior, v = _eval_batch([trees[gid].cells[waits[gid]] for gid in ask])
                for k, gid in enumerate(ask):
                    GR.receive(trees[gid], waits[gid], [float(x) for x in prior[k]], float(v[k]), gms[gid])
        for gid in live:
            t, g = trees[gid], games[gid]
            mv = GR.choose_move(t, gms[gid])
            g["moves"].append(mv)
            g["rows"].append(GR.target(t, gms[gid])[1])
            j = t.child[0][mv]
            g["cells"], g["player"], g["n"] = list(t.cells[j]), t.player[j], t.count[j]
            if t.term[j]:
                g["winner"] = 0 if t.term[j] == 3 else t.term[j]
    _CACHE["ref"] = games
    return games


def _play(n_slots, compact=False, **kw):
    """Games 0..5 -> (records sorted by (id, ply), their rows, the slots' draw counters)."""
    key = ("play", n_slots, compact, tuple(sorted(kw.items())))
    if key not in _CACHE:
        eng = SelfPlayEngine(n_slots=n_slots, num_simulations=S_ENG, c_puct=C_PUCT, seed=SEED, pv_weights=_eng_weights(),
                             search="puct", temp_plies=2, game_id_end=GAMES, compact_slots=compact, plies_per_step=25,
                             **kw)
        recs, vis, done = [], [], set()
        for _ in range(-(-GAMES // n_slots) * 8 + 2):
            eng.step()
            c = eng.counters()
            assert c["records_dropped"] == 0
            if c["records"]:
                r, v = eng.records().copy(), eng.visits().copy()
                recs.append(r)
                vis.append(v)
                done |= set(int(x) for x in r["game_id"])
            if len(done) == GAMES:
                break
            if compact:
                eng.n_active = int(eng.compact().item())
        assert done == set(range(GAMES))
        recs, vis = np.concatenate(recs), np.concatenate(vis)
        order = np.lexsort((recs["ply"], recs["game_id"]))
        _CACHE[key] = (recs[order], vis[order], eng.draws().copy())
    return _CACHE[key]


GUMBEL = dict(gumbel_considered=M_ENG)


def test_lock_step_engine_equals_the_reference():
    recs, vis, draws = _play(6, **GUMBEL)
    games = records_to_games(recs)
    ref = _reference_games()
    assert sorted(games) == list(range(GAMES))
    for gid in range(GAMES):
        r = ref[gid]
        assert games[gid]["moves"] == r["moves"], gid
        rows = vis[recs["game_id"] == gid].astype(np.int32)
        assert [list(map(int, x)) for x in rows] == r["rows"], gid
        w = r["winner"]
        assert games[gid]["z"] == [0 if w == 0 else (1 if 1 + k % 2 == w else -1) for k in range(len(r["moves"]))]
        print(f"game {gid}: {len(r['moves'])} plies, winner {w}")
    assert (draws[:, 1] == 0).all()  # main_draws is 0 everywhere
    assert (vis.max(axis=1) >= 146).all() and (vis.astype(np.int64).sum(axis=1) > 32767 - 225).all()


@pytest.mark.parametrize("compact", [False, True])
def test_lock_step_engine_gives_the_same_bytes_whatever_the_slots(compact):
    a = _play(6, **GUMBEL)
    b = _play(3, compact, **GUMBEL)  # three slots: games 3, 4, 5 are refills
    assert len(a[0]) == len(b[0]) and a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])
    assert (b[2][:, 1] == 0).all()
    if compact:
        c = _play(6, True, **GUMBEL)
        assert a[0].tobytes() == c[0].tobytes() and np.array_equal(a[1], c[1])


def test_tree_reuse_with_the_gumbel_root_raises():
    with pytest.raises(ValueError, match="gumbel_considered is not supported with tree_reuse"):
        SelfPlayEngine(n_slots=2, num_simulations=S_ENG, pv_weights=_eng_weights(), search="puct", tree_reuse=True,
                       **GUMBEL)
    with pytest.raises(ValueError, match="gumbel_considered needs search='puct'"):
        SelfPlayEngine(n_slots=2, num_simulations=S_ENG, **GUMBEL)


# ---------------------------------------------------------------- 4. flag clear
def test_flag_clear_search_leaves_the_workspace_tail_alone_and_differs_from_the_flag():
    """gz_puct_search without the flag on a workspace with room for the Gumbel region behind it,
    poison-filled: the region is untouched, and moves, rows and trees are those of a workspace
    without it."""
    L = _lib.load()
    w = _weights("f16x3")
    states, gids = _five_states(), [20, 21, 22, 23, 24]
    n, S = len(states), 16
    p = device.puct_params(S, C_PUCT, 0, 9)
    a = device.puct_search(states, gids, p, w, want_trees=True)
    fc = L.gz_puct_workspace_bytes(n, S)
    extra = 256 + L.gz_puct_gumbel_bytes(n, S, 32)
    ws = torch.full((fc + extra,), 0xA5, dtype=torch.uint8, device="cuda")
    d_states = device.to_dev(np.ascontiguousarray(states))
    d_gids = torch.as_tensor(np.asarray(gids, np.int64)).cuda()
    d_moves = torch.empty(n, dtype=torch.int32, device="cuda")
    d_rows = torch.empty(n * 225, dtype=torch.int32, device="cuda")
    d_q = torch.empty(n, dtype=torch.float64, device="cuda")
    _lib.check(L.gz_puct_search(device.ptr(d_states), device.ptr(d_gids), n, ctypes.byref(p), device.ptr(w.tensor),
                                device.ptr(ws), device.ptr(d_moves), device.ptr(d_rows), device.ptr(d_q),
                                device.stream()), "gz_puct_search")
    torch.cuda.synchronize()
    assert (ws[fc:] == 0xA5).all()
    assert np.array_equal(d_moves.cpu().numpy(), a[0]) and np.array_equal(d_rows.cpu().numpy().reshape(n, 225), a[1])
    assert d_q.cpu().numpy().tobytes() == a[2].tobytes()
    _same_trees(device._puct_trees(L, ws, n, S), a[3])
    assert (a[1].sum(axis=1)[states["over"] == 0] == S).all()  # visit counts, not a scaled policy
    # and a Gumbel search on that workspace, then a plain one again: the plain bytes once more
    g = device.puct_search(states, gids, device.puct_params(S, C_PUCT, 0, 9, gumbel_considered=16), w)
    assert not np.array_equal(g[1], a[1])
    b = device.puct_search(states, gids, p, w, want_trees=True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    _same_trees(a[3], b[3])


def _plain_engine(reuse=False, **kw):
    return SelfPlayEngine(n_slots=4, num_simulations=S_ENG, c_puct=C_PUCT, seed=SEED, pv_weights=_eng_weights(),
                          search="puct", temp_plies=2, plies_per_step=25, tree_reuse=reuse,
                          rounds_per_step=25 * (S_ENG + 1) if reuse else None, **kw)


def _pending_rows(eng):
    lay = (ctypes.c_size_t * 4)()
    assert eng.lib.gz_selfplay_puct_layout(4, S_ENG, 0, lay) == 0
    return eng.d_puct_ws[lay[0]:lay[0] + 4 * 200 * 225 * 2].view(torch.int16).view(4, 200, 225)


def _same_steps(eng, ref, big, fc, steps):
    """eng (on the poisoned buffer `big`) and ref step alike: records, rows, boards, pending rows
    of the plies played; the tail of big stays poison."""
    games = 0
    for _ in range(steps):
        eng.step()
        ref.step()
        torch.cuda.synchronize()
        assert (big[fc:] == 0xA5).all()
        ra, rb = eng.records(), ref.records()
        # (games that end in the same ply append their records in no fixed order)
        oa, ob = np.lexsort((ra["ply"], ra["game_id"])), np.lexsort((rb["ply"], rb["game_id"]))
        assert ra[oa].tobytes() == rb[ob].tobytes() and np.array_equal(eng.visits()[oa], ref.visits()[ob])
        games += len(set(ra["game_id"].tolist()))
        sa, ga = eng.boards()
        sb, gb = ref.boards()
        assert sa.tobytes() == sb.tobytes() and np.array_equal(ga, gb)
        pa, pb = _pending_rows(eng), _pending_rows(ref)
        for s in range(4):
            k = int(sa["n_moves"][s])
            assert torch.equal(pa[s, :k], pb[s, :k])
            assert (pa[s, :k].sum(dim=1) == S_ENG).all()  # visit counts, not a scaled policy
        if games >= 2:
            break
    assert games >= 2  # records of finished games were compared


def test_flag_clear_engine_leaves_the_workspace_tail_alone():
    L = _lib.load()
    eng, ref = _plain_engine(), _plain_engine()
    fc = eng.d_puct_ws.numel()
    assert fc == L.gz_selfplay_puct_workspace_bytes(4, S_ENG)
    big = torch.full((fc + 256 + L.gz_puct_gumbel_bytes(4, S_ENG, 32),), 0xA5, dtype=torch.uint8, device="cuda")
    eng.d_puct_ws = big
    _same_steps(eng, ref, big, fc, 9)


def test_own_clock_rounds_after_a_gumbel_run_on_the_same_buffer():
    """A Gumbel ply leaves its note with the buffer's address; flag-clear tree-reuse rounds with
    root noise on that buffer (they begin no search through gz_puct_begin) must be the rounds
    of a fresh buffer: the noise mixed into every new root, nothing written past the flag-clear
    size."""
    L = _lib.load()
    noise = dict(dirichlet_alpha=0.3, noise_eps=0.25)
    eng, ref = _plain_engine(True, **noise), _plain_engine(True, **noise)
    fc = eng.d_puct_ws.numel()
    g = SelfPlayEngine(n_slots=4, num_simulations=S_ENG, c_puct=C_PUCT, seed=SEED, pv_weights=_eng_weights(),
                       search="puct", plies_per_step=2, gumbel_considered=M_ENG)
    big = torch.full((fc + 256 + L.gz_puct_gumbel_bytes(4, S_ENG, 32),), 0xA5, dtype=torch.uint8, device="cuda")
    assert g.d_puct_ws.numel() <= big.numel()
    g.d_puct_ws = big
    g.step()
    torch.cuda.synchronize()
    assert not (big[fc:] == 0xA5).all()  # (the Gumbel run used its region)
    big[fc:] = 0xA5
    eng.d_puct_ws = big
    eng._puct_reset()
    _same_steps(eng, ref, big, fc, 9)


# ---------------------------------------------------------------- 5. argument errors
def _raw(mc=16, cv=50.0, cs=0.5, gsc=1.0, flags=0, S=8):
    return _lib.PuctGumbelParams(S, 0, C_PUCT, 1, _lib.GZ_PV_F16X3, _lib.GZ_PUCT_GUMBEL | flags, 0.3, 0.25, 4, 0, 4, 0,
                                 0.5, 2.0, mc, 0, cv, cs, gsc)


def test_argument_errors_launch_nothing():
    L = _lib.load()
    n, S = 2, 8
    ws = torch.full((L.gz_selfplay_puct_workspace_bytes(n, S) + 8192,), 0x5A, dtype=torch.uint8, device="cuda")
    before = ws.clone()
    ptr = ctypes.c_void_p(ws.data_ptr())
    bad = [(_raw(mc=0), b"the Gumbel root needs"), (_raw(mc=33), b"the Gumbel root needs"),
           (_raw(cv=float("nan")), b"the Gumbel root needs"), (_raw(cs=-1.0), b"the Gumbel root needs"),
           (_raw(gsc=9.0), b"the Gumbel root needs")]
    bad += [(_raw(flags=f), b"the Gumbel root with") for f in (_lib.GZ_PUCT_ROOT_NOISE, _lib.GZ_PUCT_LEAF_BATCH,
                                                               _lib.GZ_PUCT_PLAYOUT_CAP, _lib.GZ_PUCT_FORCED_PLAYOUTS)]
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
    good = _raw()
    pp = ctypes.cast(ctypes.pointer(good), ctypes.POINTER(_lib.PuctParams))
    assert L.gz_selfplay_puct_rounds(ptr, n, pp, ptr, ptr, 1, ptr, 16, ptr, ptr, None) == -1
    assert b"the Gumbel root with tree reuse" in L.gz_last_error()
    assert L.gz_selfplay_puct_rounds_active(ptr, n, n, pp, ptr, ptr, 1, ptr, 16, ptr, ptr, None) == -1
    assert b"the Gumbel root with tree reuse" in L.gz_last_error()
    mp = _lib.PuctMatchParams(ctypes.cast(ctypes.pointer(good), ctypes.c_void_p), (ctypes.c_void_p * 2)(ptr, ptr),
                              (ctypes.c_int32 * 2)(_lib.GZ_PV_F16X3, _lib.GZ_PV_F16X3), 0, 0)
    assert L.gz_puct_match_run(ptr, n, n, ctypes.byref(mp), ptr, 1, ptr, 16, ptr, ptr, None) == -1
    assert b"the Gumbel root is not supported in a match" in L.gz_last_error()
    torch.cuda.synchronize()
    assert torch.equal(ws, before)


# ---------------------------------------------------------------- 6. the rows as targets
def test_rows_train():
    from gzero.train import DeviceDataset
    from test_gpu_pi import _same_bits
    recs, vis, _ = _play(6, **GUMBEL)
    pick = np.linspace(0, len(recs) - 1, 12).astype(int)
    rows, rec = np.ascontiguousarray(vis[pick]), recs[pick].copy()
    base = rows.astype(np.float32) / rows.astype(np.int64).sum(axis=1).astype(np.float32)[:, None]
    ds = DeviceDataset(rec, use_augmentation=False, visits=rows)
    assert ds.soft and _same_bits(ds.materialize()[1].cpu().numpy(), base)


def test_training_iteration_with_the_gumbel_root():
    import gzero.train as gtrain
    import training
    from test_gpu_puct_train import _model
    model = _model()
    trainer = gtrain.DeviceTrainer(model)
    out = training.run_iteration(model, trainer, 0, 4, num_simulations=8, seed=5, search="puct", gumbel_considered=4,
                                 verbose=False, epochs=1)
    assert not out.get("skipped") and np.isfinite(out["train_loss"]) and np.isfinite(out["val_loss"])
    with pytest.raises(ValueError, match="gumbel_considered needs search='puct'"):
        training.run_iteration(model, trainer, 0, 4, num_simulations=8, seed=5, gumbel_considered=4, verbose=False)
