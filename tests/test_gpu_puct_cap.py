"""Playout cap randomization on the GPU (GZ_PUCT_PLAYOUT_CAP: csrc/gz_puct.hip) against
the plain-Python restatement in tests/puct_cap_ref.py: the step API ply by ply, the
self-play engine against the step API, independence of the slot count, the round cut
and compaction, neutrality of the flag at p = 1 and at F = S, the root noise on full
plies only, gz_puct_cap_full, the training iteration and the exported symbols.

The weights are the init weights with the policy FC scaled by 128, as tools/puct_bench.py
sharpens its prior: under the init weights' nearly flat prior no child of a 16-simulation
root collects the F + 1 = 4 visits that give a fast ply nothing left to do.

A move the search picks always has a child (every simulation passes through a root child,
so the visit row is never empty), which means the engine itself never makes a fresh root
inside a game.  The step-API run therefore has a seventh row: game 2 again, whose first
move is forced to a cell the fast search at ply 0 never tried."""
import ctypes
import os

import numpy as np
import pytest
import torch

import puct_cap_ref as CR
import puct_noise_ref as NR
import puct_ref as R
from conftest import REPO
from gzero import _lib, boards, device, weights
from gzero.boards import RECORD_DTYPE
from gzero.selfplay import SelfPlayEngine, records_to_games
from test_gpu_puct import C_PUCT, _assert_tree, _state

pytestmark = pytest.mark.gpu

S, F, PROB, TEMP, SEED = 16, 3, 0.5, 6, 7
GIDS = (0, 1, 2, 3, 4, 5)
FORCED = 2          # the game id of the seventh row, whose ply-0 move is forced
REF_PLIES = 9       # plies that are compared with the reference, tree by tree
POLICY_SCALE = 128.0
ALPHA, EPS = 0.3, 0.25

_CACHE = {}


def _weights():
    if "w" not in _CACHE:
        sd = weights.init_state_dict(0)
        sd["policy_fc.weight"] = sd["policy_fc.weight"] * POLICY_SCALE
        sd["policy_fc.bias"] = sd["policy_fc.bias"] * POLICY_SCALE
        _CACHE["w"] = device.PVWeights(weights.pack_pv_weights(sd), "f16x3")
    return _CACHE["w"]


def _evalf(cells, player):
    """The reference's evaluator: gz_pv_forward of the one board (a row's result does not
    depend on the other rows of its batch), kept per board."""
    table = _CACHE.setdefault("evals", {})
    cells = tuple(int(x) for x in cells)
    if cells not in table:
        bl, wh = boards.cells_to_words(np.array(cells, np.int8)[None])
        _, v, _, prior = device.pv_forward(_weights(), boards.leaf_words(bl, wh), want_prior=True)
        table[cells] = ([float(x) for x in prior[0]], float(v[0]))
    return table[cells]


def _snap(t):
    """A copy of a reference tree (the search goes on in place on the original)."""
    out = R.Tree()
    for f in ("parent", "move", "term", "visits", "W", "prior", "value", "cells", "player", "count"):
        setattr(out, f, list(getattr(t, f)))
    out.child = [dict(c) for c in t.child]
    return out


def _cold(visits_row, cells):
    """The first empty cell the search never tried."""
    return next(c for c in range(225) if cells[c] == 0 and visits_row[c] == 0)


def _reference(noise):
    """puct_cap_ref.play_game of games 0..5 and of the forced row, REF_PLIES plies each:
    per row dict(moves, rows, rounds, fulls, plies = [(tree before the move, tree after
    the re-root, info)])."""
    key = ("ref", noise)
    if key not in _CACHE:
        out = []
        for row, gid in enumerate(GIDS + (FORCED,)):
            plies = []
            nz = NR.Noise(SEED, gid, ALPHA, EPS) if noise else None
            force = (lambda ply, t: _cold(t.root_visits(), t.cells[0]) if ply == 0 else None) if row == len(GIDS) \
                else None
            moves, rows, z, rounds, fulls = CR.play_game(
                SEED, gid, S, F, PROB, C_PUCT, TEMP, _evalf, noise=nz, max_plies=REF_PLIES, force=force,
                on_ply=lambda ply, b, a, info: plies.append((_snap(b), _snap(a), dict(info))))
            out.append(dict(moves=moves, rows=rows, rounds=rounds, fulls=fulls, plies=plies))
        _CACHE[key] = out
    return _CACHE[key]


def _params(noise=False, fast=F, prob=PROB):
    return device.puct_params(S, C_PUCT, TEMP, SEED, "f16x3", dirichlet_alpha=ALPHA if noise else None,
                              noise_eps=EPS, fast_simulations=fast, full_prob=prob)


def _drive(noise, max_plies):
    """Games 0..5 and the forced row through PuctStepper + reroot with gz_pv_forward as the
    evaluator, as test_gpu_puct_reuse._drive_games: per row dict(moves, rows, took: rounds
    per move, evals: evaluations per move, remaining: the count reroot returned after each
    move, before / after: the exported trees of the first REF_PLIES plies)."""
    key = ("drive", noise, max_plies)
    if key in _CACHE:
        return _CACHE[key]
    w = _weights()
    gids = GIDS + (FORCED,)
    n = len(gids)
    st = device.PuctStepper(np.concatenate([_state(np.zeros(225, np.int8))] * n), gids, _params(noise))
    d_probs = torch.empty(n * 225, dtype=torch.float32, device="cuda")
    d_prior = torch.empty(n * 225, dtype=torch.float64, device="cuda")
    out = [dict(moves=[], rows=[], took=[], evals=[], remaining=[], before=[], after=[]) for _ in range(n)]

    def forward_backup():
        _, d_value, _ = device.pv_forward_dev(w, st.d_leaves, n, d_probs=d_probs, d_prior=d_prior)
        st.backup(d_prior, d_value)
        return st.d_active.cpu().numpy()

    rem = st.remaining()  # B + 1 of every fresh root
    live = np.ones(n, bool)
    for ply in range(max_plies):
        took = np.maximum(rem, 1)  # (an inherited root at or past its budget still takes the round it is picked in)
        evals = np.zeros(n, np.int64)
        if st.d_active.cpu().numpy().any():  # fresh roots wait for their evaluation
            evals += forward_backup()
        left = st.remaining()
        assert (left[live] == np.maximum(rem - evals, 0)[live]).all()
        for rnd in range(int(left.max())):
            st.select()
            active = forward_backup()
            assert not active[left <= rnd].any(), "a game at its budget has no leaf"
            evals += active
        assert not st.remaining().any()
        moves, visits, _ = st.finish()
        if (moves < 0).all():
            break
        if ply == 0:
            moves[n - 1] = _cold(visits[n - 1], np.zeros(225, np.int8))
        before = st.trees() if ply < REF_PLIES else None
        for g in range(n):
            live[g] = moves[g] >= 0
            if live[g]:
                o = out[g]
                o["moves"].append(int(moves[g]))
                o["rows"].append(visits[g].copy())
                o["took"].append(int(took[g]))
                o["evals"].append(int(evals[g]))
                if before:
                    o["before"].append(before[g])
        rem = st.reroot(moves)
        after = st.trees() if ply < REF_PLIES else None
        for g in range(n):
            if live[g]:
                out[g]["remaining"].append(int(rem[g]))
                if after:
                    out[g]["after"].append(after[g])
    _CACHE[key] = out
    return out


def _assert_tree_and_priors(gpu, ref):
    _assert_tree(gpu, ref)
    for k, t in enumerate(ref.term):
        if t == 0 and ref.prior[k] is not None:
            assert [float(x) for x in gpu["prior"][k]] == list(ref.prior[k]), k  # float64, bit for bit


def _compare_with_reference(noise):
    ref, got = _reference(noise), _drive(noise, REF_PLIES if noise else 200)
    for row, (r, g) in enumerate(zip(ref, got)):
        k = len(r["moves"])
        assert k == REF_PLIES or len(g["moves"]) == k  # (a game that ended earlier ended in both)
        assert g["moves"][:k] == r["moves"], row
        assert [list(x) for x in g["rows"][:k]] == r["rows"], row
        assert g["took"][:k] == r["rounds"], row
        for ply, (before, after, info) in enumerate(r["plies"]):
            _assert_tree_and_priors(g["before"][ply], before)
            if after.prior[0] is None:  # a fresh root that waits for its evaluation
                t = g["after"][ply]
                assert t["n_nodes"] == 1 and t["n_evals"] == 0 and list(t["visits"]) == [0]
                assert tuple(int(x) for x in boards.words_to_cells(t["board"][:, :8], t["board"][:, 8:])[0]) == \
                    after.cells[0]
            else:
                _assert_tree_and_priors(g["after"][ply], after)
            assert g["remaining"][ply] == info["remaining"], (row, ply)
            v, B = info["inherited"], info["budget"]
            want = B if v is None or v < B + 1 else v - 1
            assert int(g["rows"][ply].sum()) == want, (row, ply)
            assert g["evals"][ply] <= g["took"][ply]
            if v is not None and v >= B + 1:
                assert g["evals"][ply] == 0 and g["took"][ply] == 1
    return ref, got


# ---------------------------------------------------------------- 1. step API vs the reference
def test_step_api_equals_the_reference():
    ref, got = _compare_with_reference(False)
    zero = after_fast = fresh = 0
    for row, r in enumerate(ref):
        for ply, (_, _, info) in enumerate(r["plies"]):
            v, B = info["inherited"], info["budget"]
            if not info["full"] and v is not None and v >= F + 1:
                zero += 1
            if info["full"] and v is not None and ply > 0 and not r["fulls"][ply - 1]:
                after_fast += 1
            if v is None and ply > 0 and not r["fulls"][ply - 1]:
                fresh += 1
                assert row == len(GIDS) and ply == 1 and got[row]["took"][1] == B + 1
    # fresh roots at ply 0 of both kinds
    assert [r["fulls"][0] for r in ref[:6]] == [True, True, False, False, False, True]
    assert [g["took"][0] for g in got[:6]] == [S + 1, S + 1, F + 1, F + 1, F + 1, S + 1]
    print(f"cases: zero-simulation plies {zero}, full after fast {after_fast}, fresh after fast {fresh}")
    assert zero >= 1 and after_fast >= 1 and fresh >= 1


# ---------------------------------------------------------------- 2. the engine vs the step API
def _play(n_slots, rounds_per_step, compact=False, **kw):
    """Games 0..5 on a reuse engine -> (records sorted by (id, ply), visit rows, per-slot
    statistics of an engine that never compacted, else None)."""
    key = ("play", n_slots, rounds_per_step, compact, tuple(sorted(kw.items())))
    if key not in _CACHE:
        n_games = len(GIDS)
        eng = SelfPlayEngine(n_slots=n_slots, num_simulations=S, c_puct=C_PUCT, seed=SEED, pv_weights=_weights(),
                             search="puct", temp_plies=TEMP, tree_reuse=True, rounds_per_step=rounds_per_step,
                             game_id_end=n_games, compact_slots=compact, **kw)
        recs, vis, done, steps = [], [], 0, 0
        max_steps = -(-n_games // n_slots) * 200 * (S + 1) // eng.rounds_per_step + 2
        while done < n_games and steps < max_steps:
            eng.step()
            steps += 1
            c = eng.counters()
            assert c["records_dropped"] == 0
            done += int(c["games"])
            if c["records"]:
                recs.append(eng.records().copy())
                vis.append(eng.visits().copy())
            if compact:
                eng.n_active = int(eng.compact().item())
        assert done == n_games, (done, steps)
        recs, vis = np.concatenate(recs), np.concatenate(vis)
        order = np.lexsort((recs["ply"], recs["game_id"]))
        _CACHE[key] = (recs[order], vis[order], None if compact else eng.draws())
    return _CACHE[key]


CAP = dict(fast_simulations=F, full_prob=PROB)


def test_engine_equals_the_step_api():
    recs, vis, draws = _play(6, None, **CAP)
    games = records_to_games(recs)
    driven = _drive(False, 200)
    assert sorted(games) == list(GIDS)
    _, _, plain = _play(6, None)
    plain_games = records_to_games(_play(6, None)[0])
    for gid in GIDS:
        d = driven[gid]
        assert d["moves"] == games[gid]["moves"], gid
        assert np.array_equal(np.array(d["rows"]), vis[recs["game_id"] == gid].astype(np.int32)), gid
        assert draws[gid][0] == sum(d["evals"]) and draws[gid][1] == min(len(d["moves"]), TEMP), gid
        assert draws[gid][2] == sum(d["took"]), gid
        # per move the capped game is cheaper than the uncapped game of the same id ...
        assert draws[gid][2] / len(d["moves"]) < plain[gid][2] / len(plain_games[gid]["moves"]), gid
        print(f"game {gid}: {len(d['moves'])} plies in {draws[gid][2]} rounds; uncapped "
              f"{len(plain_games[gid]['moves'])} plies in {plain[gid][2]} rounds")
    # ... and so are the six games together (a single game's length is not the cap's to decide)
    assert draws[:, 2].sum() < plain[:, 2].sum()


# ---------------------------------------------------------------- 3. independence
@pytest.mark.parametrize("compact", [False, True])
def test_games_do_not_depend_on_slots_round_cut_or_compaction(compact):
    a = _play(6, 17, **CAP)
    b = _play(3, 5, compact, **CAP)  # three slots: games 3, 4, 5 are refills
    assert len(a[0]) == len(b[0]) and a[0].tobytes() == b[0].tobytes()
    assert np.array_equal(a[1], b[1])
    if compact:
        c = _play(6, 17, True, **CAP)
        assert a[0].tobytes() == c[0].tobytes() and np.array_equal(a[1], c[1])


# ---------------------------------------------------------------- 4. flag neutrality
@pytest.mark.parametrize("fast,prob", [(F, 1.0), (S, 0.0)])
def test_the_flag_at_its_neutral_settings_changes_nothing(fast, prob):
    a = _play(6, None)
    b = _play(6, None, fast_simulations=fast, full_prob=prob)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert (a[1].astype(np.int64).sum(axis=1) == S).all()


# ---------------------------------------------------------------- 5. noise
def test_noise_is_mixed_into_full_roots_only():
    ref, got = _compare_with_reference(True)
    mixed = plain = 0
    for row, (r, g) in enumerate(zip(ref, got)):
        gid = (GIDS + (FORCED,))[row]
        for ply, (before, _, info) in enumerate(r["plies"]):
            raw = _evalf(before.cells[0], None)[0]
            have = [float(x) for x in g["before"][ply]["prior"][0]]
            if info["full"]:
                want = NR.mix(raw, list(before.cells[0]), SEED, gid, ply, ALPHA, EPS)
                assert have == want and have != raw, (row, ply)
                mixed += 1
            else:  # the evaluated row (a fresh root) or the carried one (inherited, also from a full ply)
                assert have == raw, (row, ply)
                plain += 1
    assert mixed >= 6 and plain >= 6
    # the noise changes the games
    assert [g["moves"] for g in got] != [g["moves"][:REF_PLIES] for g in _drive(False, 200)]


# ---------------------------------------------------------------- 6. gz_puct_cap_full
def test_cap_full_on_the_engines_records():
    recs, vis, _ = _play(6, None, **CAP)
    d_recs = torch.from_numpy(np.frombuffer(recs.tobytes(), np.uint8).copy()).cuda()
    full = device.cap_full(d_recs, SEED, PROB).cpu().numpy()
    want = np.array([CR.is_full(SEED, int(g), int(p), PROB) for g, p in zip(recs["game_id"], recs["ply"])])
    assert full.dtype == np.bool_ and np.array_equal(full, want) and 0 < full.sum() < len(recs)
    sums = vis.astype(np.int64).sum(axis=1)
    first = recs["ply"] == 0
    assert (sums[first & full] == S).all() and (sums[first & ~full] == F).all()
    assert (sums[full] == S).all()  # an inherited root never holds more than S visits
    assert (sums[~full] >= F).all() and (sums[~full] > F).any()
    assert np.array_equal(device.cap_full(d_recs, SEED, 0.0).cpu().numpy(), np.zeros(len(recs), bool))
    assert np.array_equal(device.cap_full(d_recs, SEED, 1.0).cpu().numpy(), np.ones(len(recs), bool))
    # 300 records: more than one block
    many = torch.from_numpy(np.frombuffer(np.concatenate([recs] * (300 // len(recs) + 1))[:300].tobytes(),
                                          np.uint8).copy()).cuda()
    assert np.array_equal(device.cap_full(many, SEED, PROB).cpu().numpy(), np.resize(want, 300))


# ---------------------------------------------------------------- 7. training
def test_training_iteration_trains_on_the_full_plies(monkeypatch):
    import gzero.train as gtrain
    import training
    from test_gpu_puct_train import _model
    n_games, sims, seed, it = 4, 8, 11, 3
    model = _model()
    trainer = gtrain.DeviceTrainer(model)
    seen = {}
    real = gtrain.DeviceDataset

    class spy(real):  # (a class: gzero.train tests its datasets with isinstance)
        def __init__(self, d, *a, **k):
            seen["records"] = np.frombuffer(d.cpu().numpy().tobytes(), RECORD_DTYPE)
            seen["visits"] = k["visits"].cpu().numpy().view(np.uint16)
            seen["n"] = k["n_records"]
            super().__init__(d, *a, **k)

    # the iteration's games, collected first: the training below changes the weights
    base = it * n_games
    d, d_vis, n, st = training.selfplay_puct_device(n_games, num_simulations=sims, seed=seed, game_id_base=base,
                                                    model=model, temp_plies=TEMP, tree_reuse=True, fast_simulations=3,
                                                    full_prob=0.5)
    recs = np.frombuffer(d.cpu().numpy().tobytes(), RECORD_DTYPE)
    vis = d_vis.cpu().numpy().view(np.uint16)
    monkeypatch.setattr(gtrain, "DeviceDataset", spy)
    out = training.run_iteration(model, trainer, it, n_games, num_simulations=sims, seed=seed, search="puct",
                                 tree_reuse=True, fast_simulations=3, full_prob=0.5, temp_plies=TEMP, verbose=False,
                                 epochs=1)
    mask = np.array([CR.is_full(seed, int(g), int(p), 0.5) for g, p in zip(recs["game_id"], recs["ply"])])
    assert out["records_played"] == n == len(recs) and st["full_records"] == int(mask.sum())
    assert out["records"] == int(mask.sum()) < out["records_played"]
    assert seen["n"] == out["records"]
    assert seen["records"].tobytes() == recs[mask].tobytes() and np.array_equal(seen["visits"], vis[mask])
    assert (seen["visits"].astype(np.int64).sum(axis=1) == sims).all()
    assert not out.get("skipped") and np.isfinite(out["train_loss"]) and np.isfinite(out["val_loss"])


# ---------------------------------------------------------------- 8. exports
def test_new_symbols_are_exported_with_their_signatures():
    L = _lib.load()
    hdr = open(os.path.join(REPO, "include", "gzero.h")).read()
    assert ("int gz_puct_cap_full(const gz_record* d_records, int32_t n, uint64_t seed, double full_prob, "
            "uint8_t* d_full,") in hdr
    assert "int gz_puct_cap_full_host(uint64_t seed, int64_t game_id, int32_t ply, double full_prob);" in hdr
    assert _lib.SIGNATURES["gz_puct_cap_full"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64,
                                                                  ctypes.c_double, ctypes.c_void_p, ctypes.c_void_p])
    assert _lib.SIGNATURES["gz_puct_cap_full_host"] == (ctypes.c_int, [ctypes.c_uint64, ctypes.c_int64,
                                                                       ctypes.c_int32, ctypes.c_double])
    for name in ("gz_puct_cap_full", "gz_puct_cap_full_host"):
        assert hasattr(L, name)
    assert ctypes.sizeof(_lib.PuctCapParams) == 72 and _lib.GZ_PUCT_PLAYOUT_CAP == 4
    # the device path and the host path decide alike
    recs = np.zeros(64, RECORD_DTYPE)
    recs["game_id"] = np.arange(64) * 7919 + (1 << 33)
    recs["ply"] = np.arange(64) * 3
    d = torch.from_numpy(np.frombuffer(recs.tobytes(), np.uint8).copy()).cuda()
    got = device.cap_full(d, 99, 0.25).cpu().numpy()
    assert list(got) == [bool(L.gz_puct_cap_full_host(99, int(g), int(p), 0.25))
                         for g, p in zip(recs["game_id"], recs["ply"])]
