"""Playout cap randomization in the PUCT search, without a GPU: the full-or-fast decision
of the library's host function against tests/puct_cap_ref.py and gzero/rng.py, the
reference at its two neutral settings against tests/puct_reuse_ref.py, the row sums and
rounds per move of mixed play, and the argument checks of the library and of Python."""
import ctypes
import os

import pytest

import puct_cap_ref as CR
import puct_reuse_ref as RR
from conftest import REPO
from gzero import _lib, device, rng
from test_gpu_puct import C_PUCT, make_synth

S, F, PROB, TEMP, SEED = 16, 3, 0.5, 6, 7
NEW_ENTRY_POINTS = ("gz_puct_cap_full", "gz_puct_cap_full_host")


# ---------------------------------------------------------------- 1. the decision
def test_pin_vector():
    key = rng.stream_key(7, 3, 5, 0x50434150)
    assert key == 0x36fbf93649ff6b58
    assert rng.draw(key, 0) == 0xb2a4291f29e0bfe8
    assert rng.to_unit(rng.draw(key, 0)) == 0.6978173924525234
    L = _lib.load()
    # fast at p = 0.5; the comparison is strict on both sides of the unit value
    assert L.gz_puct_cap_full_host(7, 3, 5, 0.5) == 0 and not CR.is_full(7, 3, 5, 0.5)
    assert L.gz_puct_cap_full_host(7, 3, 5, 0.6978173924525234) == 0 and not CR.is_full(7, 3, 5, 0.6978173924525234)
    assert L.gz_puct_cap_full_host(7, 3, 5, 0.6978173924525235) == 1 and CR.is_full(7, 3, 5, 0.6978173924525235)
    assert CR.budget(7, 3, 5, 16, 3, 0.5) == 3 and CR.budget(7, 3, 5, 16, 3, 0.75) == 16


@pytest.mark.parametrize("prob", [0.0, 0.25, 0.5, 1.0])
def test_host_function_equals_the_reference(prob):
    L = _lib.load()
    full = 0
    for game in list(range(96)) + [1 << 33, (1 << 62) + 5, 12345678901, 999]:  # 100 games x 100 plies
        for ply in range(100):
            seed = 7 if game % 2 else 0x9E3779B97F4A7C15
            got = L.gz_puct_cap_full_host(seed, game, ply, prob)
            assert got == int(CR.is_full(seed, game, ply, prob)), (game, ply)
            full += got
    if prob == 0.0:
        assert full == 0
    elif prob == 1.0:
        assert full == 10000
    else:  # (a binomial of 10 000 draws: 8 standard deviations are 4 % at most)
        assert abs(full / 10000 - prob) < 0.04


def test_the_decision_is_its_own_stream():
    """Independent of the move-sampling stream (sim 0) and of the noise stream."""
    for sim in (0, 0x4E4F4953):
        assert CR.CAP_SIM != sim
        same = sum(CR.is_full(SEED, g, p, 0.5) == (rng.to_unit(rng.draw(rng.stream_key(SEED, g, p, sim), 0)) < 0.5)
                   for g in range(20) for p in range(50))
        assert 400 < same < 600  # 1000 pairs of independent fair coins agree about half the time


def test_the_gpu_tests_games_have_both_kinds():
    """What tests/test_gpu_puct_cap.py relies on: games 0..5 at seed 7, p = 0.5."""
    first = {g: [CR.is_full(SEED, g, ply, PROB) for ply in range(9)] for g in range(6)}
    assert all(True in f and False in f for f in first.values())
    assert [g for g in range(6) if first[g][0]] == [0, 1, 5]


# ---------------------------------------------------------------- 2. the neutral settings
@pytest.mark.parametrize("fast,prob", [(3, 1.0), (S, 0.0)])
def test_neutral_settings_reproduce_the_reuse_reference(fast, prob):
    evalf = make_synth()
    for gid in (0, 1):
        want = RR.play_game(SEED, gid, S, C_PUCT, TEMP, evalf, max_plies=30)
        got = CR.play_game(SEED, gid, S, fast, prob, C_PUCT, TEMP, evalf, max_plies=30)
        assert got[:4] == want  # moves, visit rows, z, rounds per move
        assert got[4] == [prob == 1.0] * len(want[0])


# ---------------------------------------------------------------- 3. mixed play
def test_mixed_play_row_sums_and_rounds():
    evalf = make_synth(boost=(112, 113, 97), weight=40.0)  # a sharp prior: deep, narrow trees
    kinds = set()
    for gid in range(6):
        seen = []
        moves, rows, z, rounds, fulls = CR.play_game(SEED, gid, S, F, PROB, C_PUCT, TEMP, evalf, max_plies=40,
                                                     on_ply=lambda ply, b, a, info: seen.append((b, a, info)))
        assert fulls == [CR.is_full(SEED, gid, ply, PROB) for ply in range(len(moves))]
        cells = [0] * 225
        for k, m in enumerate(moves):
            before, after, info = seen[k]
            B, v = info["budget"], info["inherited"]
            assert B == (S if fulls[k] else F) and len(before.parent) <= S + 1
            assert cells[m] == 0 and rows[k][m] > 0 and not any(x for x, c in zip(rows[k], cells) if c)
            if v is None:  # a fresh root
                assert k == 0 and sum(rows[k]) == B and rounds[k] == B + 1
            elif v >= B + 1:  # no new simulation: the inherited child visits as they are
                assert sum(rows[k]) == v - 1 >= B and rounds[k] == 1 and not fulls[k]
                kinds.add("zero")
            else:
                assert sum(rows[k]) == B and rounds[k] == B + 1 - v >= 1
                kinds.add("full after fast" if fulls[k] and not fulls[k - 1] else "other")
            assert before.visits[0] == max(B + 1, v or 0)
            if k + 1 < len(moves):  # (after is searched on in place: the next ply tells what it arrived with)
                nB = S if fulls[k + 1] else F
                assert info["remaining"] == max(0, nB + 1 - seen[k + 1][2]["inherited"])
            cells[m] = 1 + k % 2
        assert sum(rounds) < (S + 1) * len(moves)
    assert kinds == {"zero", "full after fast", "other"}


def test_a_forced_move_without_a_child_gives_a_fresh_root():
    evalf = make_synth()
    gid = 2  # fast at plies 0 and 1, full at ply 2
    seen = []

    def force(ply, t):
        if ply == 0:
            return next(c for c in range(225) if c not in t.child[0])
        return None

    moves, rows, z, rounds, fulls = CR.play_game(SEED, gid, S, F, PROB, C_PUCT, TEMP, evalf, max_plies=3, force=force,
                                                 on_ply=lambda ply, b, a, info: seen.append(
                                                     ((len(a.parent), a.prior[0], a.visits[0]), info)))
    after, info = seen[0]  # (as the re-root left it: the tree is searched on in place afterwards)
    assert rows[0][moves[0]] == 0 and after == (1, None, 0)
    assert info["remaining"] == F + 1 and rounds[:2] == [F + 1, F + 1] and sum(rows[1]) == F
    assert fulls == [False, False, True] and sum(rows[2]) == S


# ---------------------------------------------------------------- 4. the library without a GPU
def _cap_params(fast, prob, S=S, flags=_lib.GZ_PUCT_PLAYOUT_CAP):
    p = _lib.PuctCapParams(S, 0, C_PUCT, 0, _lib.GZ_PV_F16X3, flags, 0.0, 0.0, 4, 0, fast, 0, prob)
    return p, ctypes.cast(ctypes.byref(p), ctypes.POINTER(_lib.PuctParams))


def _rejected(pp, word):
    """Every entry point that takes the params returns GZ_ERR_ARG and names the field."""
    L = _lib.load()
    one = ctypes.c_int64(0)
    ptr = ctypes.addressof(one)  # any non-NULL pointer: the checks come before every GPU call
    calls = (lambda: L.gz_puct_search(ptr, ptr, 1, pp, ptr, ptr, ptr, ptr, ptr, None),
             lambda: L.gz_puct_begin(ptr, ptr, 1, pp, ptr, ptr, ptr, None),
             lambda: L.gz_selfplay_puct_run(ptr, 1, pp, ptr, ptr, 1, ptr, 0, ptr, ptr, None),
             lambda: L.gz_selfplay_puct_run_active(ptr, 1, 1, pp, ptr, ptr, 1, ptr, 0, ptr, ptr, None),
             lambda: L.gz_selfplay_puct_rounds(ptr, 1, pp, ptr, ptr, 1, ptr, 0, ptr, ptr, None),
             lambda: L.gz_selfplay_puct_rounds_active(ptr, 1, 1, pp, ptr, ptr, 1, ptr, 0, ptr, ptr, None))
    for call in calls:
        assert call() == -1 and word in L.gz_last_error(), L.gz_last_error()


@pytest.mark.parametrize("fast", [0, -1, S + 1])
def test_fast_simulations_out_of_range_is_an_argument_error(fast):
    p, pp = _cap_params(fast, 0.5)  # (p owns the memory pp points at)
    _rejected(pp, b"fast_simulations")


@pytest.mark.parametrize("prob", [-0.01, 1.01, float("nan"), float("inf"), -float("inf")])
def test_full_prob_out_of_range_is_an_argument_error(prob):
    p, pp = _cap_params(3, prob)
    _rejected(pp, b"full_prob")
    L = _lib.load()
    assert L.gz_puct_cap_full(None, 1, 0, prob, None, None) == -1 and b"full_prob" in L.gz_last_error()


def test_the_cap_with_leaf_batching_or_in_a_match_is_an_argument_error():
    p, pp = _cap_params(3, 0.5, flags=_lib.GZ_PUCT_PLAYOUT_CAP | _lib.GZ_PUCT_LEAF_BATCH)
    _rejected(pp, b"leaf batching")
    L = _lib.load()
    p, pp = _cap_params(3, 0.5)
    one = ctypes.c_int64(0)
    ptr = ctypes.addressof(one)
    mp = _lib.PuctMatchParams(ctypes.cast(pp, ctypes.c_void_p), (ctypes.c_void_p * 2)(ptr, ptr),
                              (ctypes.c_int32 * 2)(_lib.GZ_PV_F16X3, _lib.GZ_PV_F16X3), 0, 0)
    assert L.gz_puct_match_run(ptr, 1, 1, ctypes.byref(mp), ptr, 1, ptr, 0, ptr, ptr, None) == -1
    assert b"playout cap" in L.gz_last_error()


def test_without_the_flag_nothing_past_the_base_struct_is_read():
    L = _lib.load()
    p, pp = _cap_params(0, float("nan"), flags=0)
    assert L.gz_puct_search(None, None, 1, pp, None, None, None, None, None, None) == -1
    err = L.gz_last_error()
    assert b"fast_simulations" not in err and b"full_prob" not in err and b"bad arguments" in err


def test_sizes_and_surface():
    L = _lib.load()
    assert ctypes.sizeof(_lib.PuctCapParams) == 72 and _lib.GZ_PUCT_PLAYOUT_CAP == 4
    assert _lib.PuctCapParams.fast_simulations.offset == 56 and _lib.PuctCapParams.full_prob.offset == 64
    hdr = open(os.path.join(REPO, "include", "gzero.h")).read()
    for name in NEW_ENTRY_POINTS:
        assert hasattr(L, name) and name in _lib.SIGNATURES and f"int {name}(" in hdr, name
    assert "#define GZ_PUCT_PLAYOUT_CAP 4" in hdr and "} gz_puct_cap_params;" in hdr
    assert L.gz_puct_cap_full(None, 0, 0, 0.5, None, None) == 0  # no record: nothing to launch
    assert L.gz_puct_cap_full(None, 1, 0, 0.5, None, None) == -1


# ---------------------------------------------------------------- 5. Python
def test_python_parameter_checks():
    p = device.puct_params(S, C_PUCT)
    assert type(p) is _lib.PuctParams and p.flags == 0  # the default: no cap, today's struct
    c = device.puct_params(S, C_PUCT, TEMP, SEED, fast_simulations=F, full_prob=PROB)
    assert type(c) is _lib.PuctCapParams and c.flags == _lib.GZ_PUCT_PLAYOUT_CAP and (c.fast_simulations, c.full_prob) == (F, PROB)
    assert c.num_simulations == S and c.temp_plies == TEMP and c.seed == SEED and device.puct_leaves(c) == 0
    assert device.puct_params(S, C_PUCT, fast_simulations=F).full_prob == 0.25
    n = device.puct_params(S, C_PUCT, dirichlet_alpha=0.3, noise_eps=0.5, fast_simulations=S, full_prob=0.0)
    assert n.flags == 5 and n.noise_alpha == 0.3 and n.noise_eps == 0.5 and (n.fast_simulations, n.full_prob) == (S, 0.0)
    assert device.with_leaves(c, None) is c and device.with_leaves(c, 1) is c
    with pytest.raises(ValueError):
        device.with_leaves(c, 2)
    for bad in (dict(fast_simulations=0), dict(fast_simulations=S + 1), dict(fast_simulations=F, full_prob=1.5),
                dict(fast_simulations=F, full_prob=float("nan")), dict(fast_simulations=F, leaves_per_round=2)):
        with pytest.raises(ValueError):
            device.puct_params(S, C_PUCT, **bad)
    import training
    from gzero.selfplay import SelfPlayEngine
    with pytest.raises(ValueError):
        SelfPlayEngine(n_slots=4, fast_simulations=F)  # needs search="puct"
    with pytest.raises(ValueError):
        SelfPlayEngine(n_slots=4, search="puct", fast_simulations=F, leaves_per_round=2, pv_weights=object())
    with pytest.raises(ValueError):
        training.run_iteration(None, None, 0, fast_simulations=F)
    with pytest.raises(ValueError):
        training.main(iterations=0, fast_simulations=F)
