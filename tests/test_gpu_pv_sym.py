"""The leaf symmetry of the PUCT search on the GPU (GZ_PUCT_LEAF_SYM; csrc/gz_sym.h,
csrc/gz_pvsym.hip, csrc/gz_puct.hip) against tests/puct_sym_ref.py.

The forward is batch-invariant (tests/test_gpu_pv_edges.py), so the reference of
gz_pv_forward_sym is map_back of device.pv_forward on the host-transformed boards, and the
reference of every search mode is the mode's existing Python reference run with
``wrap(evalf, seed)``, evalf a cached table of single-row forwards.  Every comparison is
np.array_equal / ==.

The engines are compared over their first plies: the moves (from the slot boards after
every step), the visit rows (the pending rows of the game in progress, in the workspace)
and the exported trees.  Whole games would cost the Python reference some 10,000 forwards."""
import ctypes

import numpy as np
import pytest
import torch

import puct_batch_ref as B
import puct_cap_ref as CR
import puct_match_ref as MR
import puct_noise_ref as NR
import puct_ref as R
import puct_reuse_ref as RR
import puct_sym_ref as SR
from gzero import _lib, arena, boards, device
from gzero.boards import STATE_DTYPE
from gzero.device import ptr, stream, to_dev
from gzero.selfplay import SelfPlayEngine
from test_gpu_puct import C_PUCT, _assert_tree, _clear, _five_states, _pattern_cells, _state, _thinned, _weights
from test_gpu_puct_compact import _layout
from test_gpu_puct_match import _assert_equals_drive, _sides

pytestmark = pytest.mark.gpu

SEED = 9
PRECISIONS = ("fp32", "f16x3", "f16")


def _rows_of(cells):
    return np.array([SR.pack_row(c) for c in cells], np.uint32)


def _cells_of(rows):
    return boards.words_to_cells(rows[:, :8], rows[:, 8:])


def _positions():
    """The tactical position, three thinned boards and the empty board."""
    tcells, _, _ = R.tactical_position()
    return [np.array(tcells, np.int8), _thinned(12, 7), _thinned(47, 8), _thinned(200, 9), np.zeros(225, np.int8)]


def _table_eval(w):
    """evalf(cells, player) = the single-row forward of the board (prior float64 list, value
    as (double)float32), cached per board (.cache: the boards asked for so far)."""
    cache = {}

    def evalf(cells, player):
        cells = tuple(int(x) for x in cells)
        if cells not in cache:
            _, v, _, prior = device.pv_forward(w, _rows_of([cells]), want_prior=True)
            cache[cells] = ([float(x) for x in prior[0]], float(v[0]))
        return cache[cells]

    evalf.cache = cache
    return evalf


def _assert_rows(gpu, ref):
    """_assert_tree and every prior row of an evaluated live node, float64 bit for bit."""
    _assert_tree(gpu, ref)
    for k, t in enumerate(ref.term):
        if t == 0 and ref.prior[k] is not None:
            assert [float(x) for x in gpu["prior"][k]] == list(ref.prior[k]), k


def _stored_rows_are_sym_forwards(trees, w, seed, skip_roots=False):
    """Every live node's stored prior and value = pv_forward_sym(seed) of its exported board
    (after a backup every live node is evaluated; skip_roots: the roots took the noise)."""
    sel = [np.flatnonzero((t["term"] == 0) & (np.arange(t["n_nodes"]) >= (1 if skip_roots else 0))) for t in trees]
    rows = np.concatenate([t["board"][s] for t, s in zip(trees, sel)])
    prior = np.concatenate([t["prior"][s] for t, s in zip(trees, sel)])
    value = np.concatenate([t["value"][s] for t, s in zip(trees, sel)])
    _, fv, _, fprior = device.pv_forward_sym(w, rows, seed=seed, want_prior=True)
    assert len(rows) > 0 and np.array_equal(prior, fprior) and np.array_equal(value, fv)
    return len(rows)


# ---------------------------------------------------------------- 1. gz_pv_sym
def test_pv_sym_kernel_equals_the_reference():
    one_empty = _clear(_pattern_cells(), [113])
    special = [np.zeros(225, np.int8)]
    for c in (0, 14, 210, 224):
        special += [np.eye(1, 225, c, dtype=np.int8)[0] * col for col in (1, 2)]  # a stone in each corner
    edge = np.zeros(225, np.int8)
    edge[14 * 15:] = 1      # row 14
    edge[14::15] = 2        # column 14
    special += [edge, one_empty]
    rnd = np.random.RandomState(77).randint(0, 3, (300 - len(special), 225)).astype(np.int8)
    rows = _rows_of(special + list(rnd))
    assert rows.shape == (300, 16)
    for seed in (0, 3, SEED, (1 << 64) - 1):
        got = device.pv_sym(rows, seed)
        assert got.dtype == np.uint8 and list(got) == [SR.sym_of(seed, r) for r in rows], seed
    assert device.pv_sym(rows[:1], 3)[0] == 3 and len(set(device.pv_sym(rows, 3))) == 8


# ---------------------------------------------------------------- 2. explicit d_sym
@pytest.mark.parametrize("precision", PRECISIONS)
def test_forward_sym_with_given_transforms(precision):
    w = _weights(precision)
    pos = _positions()
    cells = [p for p in pos for _ in range(8)]
    sym = np.array([t for _ in pos for t in range(8)], np.uint8)
    rows = _rows_of(cells)
    y = _rows_of([SR.transform_cells(c, int(t)) for c, t in zip(cells, sym)])
    lg, v, pr, prior = device.pv_forward_sym(w, rows, sym=sym, seed=12345, want_prior=True)
    ylg, yv, ypr, yprior = device.pv_forward(w, y, want_prior=True)
    for got, on_y in ((lg, ylg), (pr, ypr), (prior, yprior)):
        want = np.stack([SR.map_back(on_y[i], int(sym[i])) for i in range(len(rows))])
        assert got.dtype == want.dtype and np.array_equal(got, want)
    assert np.array_equal(v, yv)
    plain = device.pv_forward(w, rows, want_prior=True)
    ident = sym == 0
    for got, p in zip((lg, v, pr, prior), plain):
        assert np.array_equal(got[ident], p[ident])
    # the net is not equivariant: without this the test could pass on an identity
    differ = [i for i in range(len(rows)) if sym[i] and not np.array_equal(lg[i], plain[0][i])]
    print(f"{precision}: {len(differ)} of {int((~ident).sum())} transformed rows differ from the plain forward, "
          f"max |dlogit| {np.abs(lg - plain[0]).max():.3e}")
    assert differ
    # bits 3..7 of a transform are ignored
    lg8, v8, _ = device.pv_forward_sym(w, rows, sym=sym | 0xF8)
    assert np.array_equal(lg8, lg) and np.array_equal(v8, v)


# ---------------------------------------------------------------- 3. row-count edges
@pytest.mark.parametrize("n", [1, 257, 1000])
def test_forward_sym_with_hashed_transforms(n):
    w = _weights("f16x3")
    cells = np.random.RandomState(n).randint(0, 3, (n, 225)).astype(np.int8)
    cells[0] = 0
    rows = _rows_of(cells)
    sym = device.pv_sym(rows, SEED)
    lg, v, pr, prior = device.pv_forward_sym(w, rows, seed=SEED, want_prior=True)
    y = _rows_of([SR.transform_cells(c, int(t)) for c, t in zip(cells, sym)])
    ylg, yv, ypr, yprior = device.pv_forward(w, y, want_prior=True)
    for got, on_y in ((lg, ylg), (pr, ypr), (prior, yprior)):
        assert np.array_equal(got, np.stack([SR.map_back(on_y[i], int(sym[i])) for i in range(n)]))
    assert np.array_equal(v, yv)
    other = device.pv_forward_sym(w, rows[:8], seed=SEED + 1)[0]
    assert n < 8 or not np.array_equal(other, lg[:8])  # the seed is read


@pytest.mark.parametrize("count", [0, 1, 63, 64])
def test_forward_sym_leaves_the_rows_past_the_count(count):
    w = _weights("f16x3")
    cap = 64
    cells = np.random.RandomState(5).randint(0, 3, (cap, 225)).astype(np.int8)
    rows = _rows_of(cells)
    d_b = torch.from_numpy(rows.view(np.int32).copy()).cuda()
    d_count = torch.tensor([count], dtype=torch.int32, device="cuda")
    d_lg = torch.full((cap * 225,), -7.5, dtype=torch.float32, device="cuda")
    d_pr = torch.full((cap * 225,), -8.5, dtype=torch.float32, device="cuda")
    d_v = torch.full((cap,), -9.5, dtype=torch.float32, device="cuda")
    d_prior = torch.full((cap * 225,), -10.5, dtype=torch.float64, device="cuda")
    device.pv_forward_sym_dev(w, d_b, cap, seed=SEED, d_count=d_count, d_logits=d_lg, d_value=d_v, d_probs=d_pr,
                              d_prior=d_prior)
    torch.cuda.synchronize()
    assert np.array_equal(d_b.cpu().numpy().view(np.uint32), rows)  # d_boards is const
    lg, v, pr, prior = device.pv_forward_sym(w, rows, seed=SEED, want_prior=True)
    for d, full, sentinel, width in ((d_lg, lg, -7.5, 225), (d_pr, pr, -8.5, 225), (d_v, v, -9.5, 1),
                                     (d_prior, prior, -10.5, 225)):
        got = d.cpu().numpy().reshape(cap, width)
        assert np.array_equal(got[:count], full.reshape(cap, width)[:count])
        assert (got[count:] == sentinel).all()


# ---------------------------------------------------------------- 4. gz_puct_search
@pytest.mark.parametrize("precision", ["f16x3", "fp32"])
def test_search_with_the_flag(precision):
    w = _weights(precision)
    S, n = 64, 5
    states, gids = _five_states(), [20, 21, 22, 23, 24]
    p = device.puct_params(S, C_PUCT, 0, SEED, precision, leaf_symmetry=True)
    moves, visits, q, trees = device.puct_search(states, gids, p, w, want_trees=True)
    evalf = _table_eval(w)
    wrapped = SR.wrap(evalf, SEED)
    for g in range(n):
        s = states[g]
        cells = [int(x) for x in boards.words_to_cells(s["black"], s["white"])]
        ref = R.search(cells, int(s["player"]), int(s["n_moves"]), S, C_PUCT, wrapped)
        _assert_rows(trees[g], ref)
        assert list(visits[g]) == ref.root_visits() and visits[g].sum() == S
        assert int(moves[g]) == R.choose_move(ref, 0, SEED, gids[g])[0]
        assert float(q[g]) == R.root_q(ref)
    count = _stored_rows_are_sym_forwards(trees, w, SEED)
    print(f"{precision}: {count} nodes, {len(evalf.cache)} distinct transformed boards evaluated by the reference")

    # the same search through the step API: the caller evaluates with gz_pv_forward_sym
    st = device.PuctStepper(states, gids, p)
    d_probs = torch.empty(n * 225, dtype=torch.float32, device="cuda")
    d_prior = torch.empty(n * 225, dtype=torch.float64, device="cuda")
    for rnd in range(S + 1):
        if rnd:
            st.select()
        _, d_value, _ = device.pv_forward_sym_dev(w, st.d_leaves, n, seed=SEED, d_probs=d_probs, d_prior=d_prior)
        st.backup(d_prior, d_value)
    m2, v2, q2 = st.finish()
    assert np.array_equal(m2, moves) and np.array_equal(v2, visits) and np.array_equal(q2, q)
    for a, b in zip(st.trees(), trees):
        assert a["n_nodes"] == b["n_nodes"]
        for key in ("W", "visits", "value", "parent", "move_of", "term", "board"):
            assert np.array_equal(a[key], b[key]), key
        live = a["term"] == 0
        assert np.array_equal(a["prior"][live], b["prior"][live])
    # ... and through PuctStepper.evaluate, which reads the flag
    st = device.PuctStepper(states, gids, p)
    for rnd in range(S + 1):
        if rnd:
            st.select()
        st.backup(*st.evaluate(w))
    assert np.array_equal(st.finish()[1], visits)

    # the flag changes the search
    off = device.puct_params(S, C_PUCT, 0, SEED, precision)
    _, visits0, _, trees0 = device.puct_search(states, gids, off, w, want_trees=True)
    changed = [g for g in range(n) if not np.array_equal(trees[g]["prior"][0], trees0[g]["prior"][0])]
    print(f"{precision}: root rows of games {changed} differ from the flag-clear search; "
          f"visit rows differ in {[g for g in range(n) if not np.array_equal(visits[g], visits0[g])]}")
    assert changed and not np.array_equal(visits, visits0)


# ---------------------------------------------------------------- 5. leaf batching
def test_leaf_batching_with_the_flag():
    w = _weights("f16x3")
    S, K = 33, 4
    states = np.concatenate([_state(_thinned(12, 7)), _state(np.zeros(225, np.int8))])
    gids = [5, 6]
    p = device.puct_params(S, C_PUCT, 0, SEED, leaves_per_round=K, leaf_symmetry=True)
    moves, visits, q, trees = device.puct_search(states, gids, p, w, want_trees=True)
    wrapped = SR.wrap(_table_eval(w), SEED)
    for g in range(2):
        s = states[g]
        cells = [int(x) for x in boards.words_to_cells(s["black"], s["white"])]
        ref = B.search(cells, int(s["player"]), int(s["n_moves"]), S, K, C_PUCT, wrapped)
        _assert_rows(trees[g], ref.t)
        assert list(visits[g]) == ref.t.root_visits() and int(visits[g].sum()) == S
        assert int(moves[g]) == R.choose_move(ref.t, 0, SEED, gids[g])[0]
    _stored_rows_are_sym_forwards(trees, w, SEED)


# ---------------------------------------------------------------- 6. self-play
def _watch(eng, steps, plies):
    """Step the engine; per slot (game id at the start, its first `plies` moves, their visit rows)."""
    n = eng.n_slots
    st, gids0 = eng.boards()
    assert not st["n_moves"].any()
    prev = _cells_of(np.concatenate([st["black"], st["white"]], axis=1))
    moves = [[] for _ in range(n)]
    for _ in range(steps):
        eng.step()
        assert eng.counters()["records_dropped"] == 0
        st, gids = eng.boards()
        cur = _cells_of(np.concatenate([st["black"], st["white"]], axis=1))
        for s in range(n):
            assert gids[s] == gids0[s], "a game ended inside the watched plies"
            new = np.flatnonzero(cur[s] != prev[s])
            assert len(new) + len(moves[s]) == st["n_moves"][s] and len(new) <= 1
            moves[s] += [int(c) for c in new]
        prev = cur
    assert all(len(m) >= plies for m in moves)
    lay = _layout(eng)
    pend = eng.d_puct_ws[lay[0]: lay[0] + n * 200 * 225 * 2].cpu().numpy().view(np.uint16).reshape(n, 200, 225)
    trees = device._puct_trees(eng.lib, eng.d_puct_ws[lay[1]:], n, eng.puct.num_simulations)
    return [int(g) for g in gids0], [m[:plies] for m in moves], pend[:, :plies].astype(np.int64), moves, trees


def test_lockstep_selfplay_with_the_flag_and_root_noise():
    w = _weights("f16x3")
    S, n, plies, temp, seed, alpha, eps = 16, 3, 6, 2, 21, 0.3, 0.25
    eng = SelfPlayEngine(n_slots=n, num_simulations=S, c_puct=C_PUCT, seed=seed, pv_weights=w, search="puct",
                         temp_plies=temp, dirichlet_alpha=alpha, noise_eps=eps, leaf_symmetry=True)
    gids, moves, rows, _, trees = _watch(eng, plies, plies)
    wrapped = SR.wrap(_table_eval(w), seed)
    for s, gid in enumerate(gids):
        cells = [0] * 225
        noise = NR.Noise(seed, gid, alpha, eps)
        for ply in range(plies):
            ref = NR.search(cells, 1 + ply % 2, ply, S, C_PUCT, wrapped, noise)
            assert R.choose_move(ref, temp, seed, gid)[0] == moves[s][ply], (s, ply)
            assert ref.root_visits() == list(rows[s][ply]), (s, ply)
            cells[moves[s][ply]] = 1 + ply % 2
        _assert_rows(trees[s], ref)  # the workspace holds the last ply's search
    # the root's row took the noise after the map-back; every other row is the evaluator's
    _stored_rows_are_sym_forwards(trees, w, seed, skip_roots=True)
    off = SelfPlayEngine(n_slots=n, num_simulations=S, c_puct=C_PUCT, seed=seed, pv_weights=w, search="puct",
                         temp_plies=temp, dirichlet_alpha=alpha, noise_eps=eps)
    assert not np.array_equal(_watch(off, plies, plies)[2], rows)


@pytest.mark.parametrize("cap", [False, True])
def test_tree_reuse_selfplay_with_the_flag(cap):
    w = _weights("f16x3")
    S, n, plies, temp, seed, F, prob = 16, 3, 4, 2, 21, 4, 0.5
    kw = dict(fast_simulations=F, full_prob=prob) if cap else {}
    eng = SelfPlayEngine(n_slots=n, num_simulations=S, c_puct=C_PUCT, seed=seed, pv_weights=w, search="puct",
                         temp_plies=temp, tree_reuse=True, rounds_per_step=1, leaf_symmetry=True, **kw)
    # a move takes at most S + 1 rounds and is played in the round after its last simulation
    gids, moves, rows, _, trees = _watch(eng, plies * (S + 1) + 1, plies)
    wrapped = SR.wrap(_table_eval(w), seed)
    for s, gid in enumerate(gids):
        if cap:
            want = CR.play_game(seed, gid, S, F, prob, C_PUCT, temp, wrapped, max_plies=plies)
        else:
            want = RR.play_game(seed, gid, S, C_PUCT, temp, wrapped, max_plies=plies)
        assert want[0] == moves[s], s
        assert np.array_equal(np.array(want[1], np.int64), rows[s]), s
    # the trees in progress (carried and new nodes alike): every stored row is the flag's evaluation
    _stored_rows_are_sym_forwards(trees, w, seed)


def _play_out(n_slots, n_games, compacting):
    S, seed = 8, 21
    eng = SelfPlayEngine(n_slots=n_slots, num_simulations=S, c_puct=C_PUCT, seed=seed, pv_weights=_weights("f16x3"),
                         search="puct", temp_plies=4, tree_reuse=True, game_id_end=n_games, compact_slots=compacting,
                         leaf_symmetry=True)
    recs, vis, done = [], [], 0
    for _ in range(-(-n_games // n_slots) * 200 + 8):
        eng.step()
        c = eng.counters()
        assert c["records_dropped"] == 0
        if c["records"]:
            recs.append(eng.records().copy())
            vis.append(eng.visits().copy())
        done += int(c["games"])
        if done >= n_games:
            break
        if compacting:
            eng.n_active = int(eng.compact().item())
    assert done == n_games
    recs, vis = np.concatenate(recs), np.concatenate(vis)
    order = np.lexsort((recs["ply"], recs["game_id"]))
    return recs[order], vis[order]


def test_compaction_does_not_change_the_games():
    a, av = _play_out(3, 5, False)
    b, bv = _play_out(3, 5, True)
    assert sorted(set(int(g) for g in a["game_id"])) == list(range(5))
    assert a.tobytes() == b.tobytes() and av.tobytes() == bv.tobytes()


# ---------------------------------------------------------------- 7. the match
def test_match_with_the_flag():
    sides = _sides()  # init_state_dict(0) in f16x3 against init_state_dict(1) in f16
    S, temp, seed = 12, 4, 21
    m = arena.PuctMatch(sides[0], sides[1], 4, num_simulations=S, c_puct=C_PUCT, temp_plies=temp, seed=seed,
                        leaf_symmetry=True)
    m.run()
    p = {"num_simulations": S, "c_puct": C_PUCT, "temp_plies": temp, "seed": seed}
    # the driver searches every ply with gz_puct_search, side by side: the flag there is test 4's
    ref = MR.drive(range(4), sides, dict(p, leaf_symmetry=True))
    _assert_equals_drive(m, ref, S)
    plain = MR.drive(range(4), sides, p, max_plies=6)
    assert any(plain[g]["visits"][k].tolist() != ref[g]["visits"][k].tolist() for g in range(4) for k in range(6))


# ---------------------------------------------------------------- 8. the workspace
@pytest.mark.parametrize("K", [0, 4])
@pytest.mark.parametrize("flag", [False, True])
def test_nothing_past_the_workspace_is_touched(flag, K):
    lib = device.require_gpu()
    w = _weights("f16x3")
    S, n, guard = 8, 5, 4096
    states, gids = _five_states(), [1, 2, 3, 4, 5]
    p = device.puct_params(S, C_PUCT, 0, SEED, leaves_per_round=max(1, K), leaf_symmetry=flag)
    clear = lib.gz_puct_batch_workspace_bytes(n, S, K) if K else lib.gz_puct_workspace_bytes(n, S)
    size = clear + (lib.gz_puct_sym_bytes(n * max(1, K)) if flag else 0)
    assert size == device._puct_workspace_bytes(lib, n, p)
    ws = torch.full((size + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    d_states = to_dev(np.ascontiguousarray(states, dtype=STATE_DTYPE))
    d_gids = torch.as_tensor(np.asarray(gids, np.int64)).cuda()
    d_moves = torch.empty(n, dtype=torch.int32, device="cuda")
    d_visits = torch.empty(n * 225, dtype=torch.int32, device="cuda")
    d_q = torch.empty(n, dtype=torch.float64, device="cuda")
    _lib.check(lib.gz_puct_search(ptr(d_states), ptr(d_gids), n, ctypes.byref(p), ptr(w.tensor), ptr(ws), ptr(d_moves),
                                  ptr(d_visits), ptr(d_q), stream()), "gz_puct_search")
    torch.cuda.synchronize()
    tail = ws[size:].cpu().numpy()
    assert (tail == 0xA5).all()
    want = device.puct_search(states, gids, p, w)
    assert np.array_equal(d_visits.cpu().numpy().reshape(n, 225), want[1])
    if flag:  # the extra region holds the transforms of the last round's rows
        t = ws[clear: clear + n * max(1, K)].cpu().numpy()
        assert (t < 8).all()


# ---------------------------------------------------------------- 9. the Python layers
def test_agent_training_and_arena_carry_the_flag():
    import training
    from ai_agent import AIFactory
    from gomoku_board import GomokuBoard
    from gzero.train import DeviceTrainer
    from test_gpu_puct_train import _model
    ai = AIFactory.create_ai("alphazero", 1, "easy", search="puct", seed=5, game_id=2, leaf_symmetry=True)
    b0, b1 = GomokuBoard(), GomokuBoard()
    for r, c in ((7, 7), (7, 8), (8, 8)):
        b1.make_move(r, c)
    got = ai.get_moves([b0, b1], [2, 9])
    S = ai.params["num_simulations"]
    states = np.concatenate([b0.to_state(), b1.to_state()])
    w = ai.model.device_weights()
    on = device.puct_search(states, [2, 9], device.puct_params(S, ai.params["c_puct"], 0, 5, leaf_symmetry=True), w)
    off = device.puct_search(states, [2, 9], device.puct_params(S, ai.params["c_puct"], 0, 5), w)
    assert got == [(int(m) // 15, int(m) % 15) for m in on[0]]
    assert np.array_equal(ai.last_search_visits, on[1]) and not np.array_equal(on[1], off[1])

    model = _model()
    DeviceTrainer(model)
    kw = dict(num_simulations=8, seed=11, game_id_base=12, model=model, temp_plies=0)
    d1, v1, n1, st1 = training.selfplay_puct_device(4, leaf_symmetry=True, **kw)
    d0, v0, n0, _ = training.selfplay_puct_device(4, **kw)
    d2, v2, n2, _ = training.selfplay_puct_device(4, leaf_symmetry=False, **kw)
    assert st1["games"] == 4 and (v1.cpu().numpy().view(np.uint16).astype(np.int64).sum(axis=1) == 8).all()
    assert n0 == n2 and d0.cpu().numpy().tobytes() == d2.cpu().numpy().tobytes()  # the default is off
    assert v1.cpu().numpy().tobytes() != v0.cpu().numpy()[: len(v1)].tobytes() or n1 != n0
    res = arena.play_match(model, model, games=2, num_simulations=6, seed=3, leaf_symmetry=True)
    assert res["games_played"] == 2
