"""The PUCT arena without a GPU: the argument errors of gz_puct_match_run (returned
before any launch), the sizes of the two new structs, the plain-Python tally and Wilson
interval on hand-written records, and the errors of evaluate_model(search="puct")."""
import ctypes
import math

import numpy as np
import pytest

import puct_match_ref as MR
from gzero import _lib, arena
from gzero.boards import RECORD_DTYPE


def test_struct_sizes():
    assert ctypes.sizeof(_lib.PuctMatchParams) == 40
    assert ctypes.sizeof(_lib.PuctMatchTally) == 72
    assert [f[0] for f in _lib.PuctMatchTally._fields_] == list(MR.TALLY_FIELDS) == list(arena.TALLY_FIELDS)


class _Call:
    """A gz_puct_match_run call whose every argument is valid as far as the host can tell
    (the device pointers are never dereferenced before the checks pass)."""

    def __init__(self):
        self.search = _lib.PuctParams(8, 4, 1.6, 3, _lib.GZ_PV_F16X3, 0)
        self.fake = ctypes.create_string_buffer(4096)
        d = ctypes.addressof(self.fake)
        self.mp = _lib.PuctMatchParams(ctypes.addressof(self.search), (ctypes.c_void_p * 2)(d, d),
                                       (ctypes.c_int32 * 2)(_lib.GZ_PV_F16X3, _lib.GZ_PV_F16), 0, 0)
        self.args = {"slots": d, "n_slots": 4, "n_active": 4, "mp": ctypes.addressof(self.mp), "ws": d, "n_plies": 1,
                     "records": d, "cap": 800, "visits": d, "counters": d}

    def run(self, **kw):
        a = dict(self.args, **kw)
        L = _lib.load()
        return L.gz_puct_match_run(ctypes.c_void_p(a["slots"]), a["n_slots"], a["n_active"],
                                   ctypes.cast(ctypes.c_void_p(a["mp"]), ctypes.POINTER(_lib.PuctMatchParams)),
                                   ctypes.c_void_p(a["ws"]), a["n_plies"], ctypes.c_void_p(a["records"]), a["cap"],
                                   ctypes.c_void_p(a["visits"]), ctypes.c_void_p(a["counters"]), None)


def _fails(rc, word):
    msg = _lib.load().gz_last_error()
    assert rc == -1 and msg.startswith(b"gz_puct_match_run") and word in msg, (rc, msg)


@pytest.mark.parametrize("name", ["slots", "mp", "ws", "records", "visits", "counters"])
def test_null_pointer(name):
    _fails(_Call().run(**{name: None}), b"NULL" if name == "mp" else b"bad arguments")


def test_null_inside_the_params():
    c = _Call()
    c.mp.search = None
    _fails(c.run(), b"NULL")
    for sd in (0, 1):
        c = _Call()
        c.mp.d_weights[sd] = None
        _fails(c.run(), b"bad arguments")


@pytest.mark.parametrize("sd", [0, 1])
@pytest.mark.parametrize("bad", [-1, 3, 99])
def test_unknown_precision(sd, bad):
    c = _Call()
    c.mp.precision[sd] = bad
    _fails(c.run(), b"precision")


@pytest.mark.parametrize("parity", [-1, 2, 7])
def test_parity_out_of_range(parity):
    c = _Call()
    c.mp.a_black_parity = parity
    _fails(c.run(), b"a_black_parity")


@pytest.mark.parametrize("n_active", [0, -2, 5])
def test_n_active_out_of_range(n_active):
    _fails(_Call().run(n_active=n_active), b"n_active")


def test_leaf_batching_is_refused():
    c = _Call()
    c.search.flags = _lib.GZ_PUCT_LEAF_BATCH
    _fails(c.run(), b"leaf batching")
    c.search.flags = _lib.GZ_PUCT_LEAF_BATCH | _lib.GZ_PUCT_ROOT_NOISE
    _fails(c.run(), b"leaf batching")


def test_results_arguments():
    L = _lib.load()
    buf = ctypes.create_string_buffer(256)
    d = ctypes.c_void_p(ctypes.addressof(buf))
    assert L.gz_puct_match_results(d, 1, 0, 0, 1, None, None, None) == -1
    assert L.gz_puct_match_results(None, 1, 0, 0, 1, d, None, None) == -1
    assert L.gz_puct_match_results(d, 1, 2, 0, 1, d, None, None) == -1 and b"a_black_parity" in L.gz_last_error()
    assert L.gz_puct_match_results(None, 0, 0, 0, 0, d, None, None) == 0  # no records: nothing to do


def test_workspace_begins_with_the_selfplay_workspace():
    L = _lib.load()
    for n, S in ((1, 1), (5, 6), (70, 6), (4096, 200)):
        sp, pv = L.gz_selfplay_puct_workspace_bytes(n, S), L.gz_pv_workspace_bytes(n)
        al = lambda x: (x + 255) & ~255
        rows = al(n * 64) + al(n * 4) + 2 * al(n * 900) + al(n * 4) + al(n * 1800) + pv
        assert L.gz_puct_match_workspace_bytes(n, S) == sp + 2 * al(n * 4) + 256 + 2 * rows


def _records(rows):
    r = np.zeros(len(rows), RECORD_DTYPE)
    for i, (gid, ply, z) in enumerate(rows):
        r[i]["game_id"], r[i]["ply"], r[i]["z"], r[i]["player"] = gid, ply, z, 1 + ply % 2
    return r


def test_side_of():
    # parity 0: A is black in the even games
    assert [MR.side_of(g, 1, 0) for g in range(4)] == [0, 1, 0, 1]
    assert [MR.side_of(g, 2, 0) for g in range(4)] == [1, 0, 1, 0]
    assert [MR.side_of(g, 1, 1) for g in range(4)] == [1, 0, 1, 0]
    assert MR.side_of(-3, 1, 0) == 1 and MR.side_of(-4, 2, 1) == 0


def test_tally_on_hand_written_records():
    # game 10: black wins in 3 plies; 11: white wins in 2; 12: a draw; 13: black wins in 1
    recs = _records([(10, 0, 1), (10, 1, -1), (10, 2, 1), (11, 0, -1), (11, 1, 1), (12, 0, 0), (12, 1, 0),
                     (13, 0, 1)])
    t, res = MR.tally(recs, 0)  # A black in 10 and 12
    assert t == {"games": 4, "a_wins": 2, "b_wins": 1, "draws": 1, "a_wins_black": 1, "a_wins_white": 1,
                 "b_wins_black": 1, "b_wins_white": 0, "plies": 8}
    assert res == {10: 1, 11: 1, 12: 0, 13: -1}
    t, res = MR.tally(recs, 1)  # A black in 11 and 13
    assert t == {"games": 4, "a_wins": 1, "b_wins": 2, "draws": 1, "a_wins_black": 1, "a_wins_white": 0,
                 "b_wins_black": 1, "b_wins_white": 1, "plies": 8}
    assert res == {10: -1, 11: -1, 12: 0, 13: 1}
    s = arena.summarise(t)
    assert (s["wins"], s["losses"], s["draws"], s["plies"]) == (1, 2, 1, 8) and s["win_rate"] == 0.25
    assert s["wins_black"] + s["wins_white"] == s["wins"] and s["losses_black"] + s["losses_white"] == s["losses"]
    assert s["score"] == 1.5 / 4 and s["wilson95"] == arena.wilson(1.5, 4)


def test_wilson_at_the_ends():
    z2 = 1.959963984540054 ** 2
    for f in (MR.wilson, arena.wilson):
        lo, hi = f(0, 7)
        assert abs(lo) < 1e-12 and abs(hi - z2 / (7 + z2)) < 1e-12
        lo, hi = f(7, 7)
        assert abs(hi - 1) < 1e-12 and abs(lo - 7 / (7 + z2)) < 1e-12


@pytest.mark.parametrize("score,n", [(5, 10), (1, 7), (2048.5, 4096), (1.5, 4)])
def test_wilson(score, n):
    z = 1.959963984540054
    lo, hi = MR.wilson(score, n)
    # the ends are the proportions p0 at which score / n lies z standard errors away
    for p0 in (lo, hi):
        assert abs(abs(score / n - p0) - z * math.sqrt(p0 * (1 - p0) / n)) < 1e-12
    assert lo <= score / n <= hi
    a = arena.wilson(score, n)
    assert abs(a[0] - lo) < 1e-12 and abs(a[1] - hi) < 1e-12
    if (score, n) == (5, 10):
        assert abs(lo - 0.2366) < 1e-4 and abs(hi - 0.7634) < 1e-4


def test_evaluate_model_errors():
    import training
    with pytest.raises(ValueError, match="baseline"):
        training.evaluate_model(object(), None, search="puct")
    with pytest.raises(ValueError, match="search"):
        training.evaluate_model(object(), object(), search="mcts")
    with pytest.raises(ValueError, match="arena_search"):
        training.main(iterations=0, arena_search="mcts")
