"""Leaf batching with virtual loss in the PUCT search, without a GPU: the plain-Python
restatement (tests/puct_batch_ref.py) against puct_ref at K = 1, its invariants at
K > 1, two crafted inputs that make it collide and back up terminals inside a batch,
and the library's argument checks and sizes."""
import ctypes

import pytest

import puct_batch_ref as B
import puct_ref as R
from gzero import _lib

C_PUCT = 1.6


def _sparse_position():
    """Seven stones, no run longer than two, white to move."""
    cells = [0] * 225
    for c, x in ((112, 1), (113, 2), (97, 1), (128, 2), (111, 1), (127, 2), (96, 1)):
        cells[c] = x
    return cells, 2, 7


def _hash_eval(cells, player):
    """A prior that differs per board and cell, and a value in (-1, 1), from integers."""
    h = 0
    for c, x in enumerate(cells):
        if x:
            h = (h * 1000003 + c * 4 + x) % 2147483647
    w = [0.0 if x else 1.0 + ((h + 7919 * c) % 1009) / 64.0 for c, x in enumerate(cells)]
    total = sum(w)
    return [x / total for x in w], ((h % 2001) - 1000) / 1024.0


# ---------------------------------------------------------------- 1. K = 1 is puct_ref.search
@pytest.mark.parametrize("S", [1, 2, 40])
@pytest.mark.parametrize("case", ["tactical_uniform", "sparse_hash"])
def test_one_leaf_per_round_is_the_unbatched_search(S, case):
    if case == "tactical_uniform":
        (cells, player, n_moves), evalf = R.tactical_position(), R.uniform_eval
    else:
        (cells, player, n_moves), evalf = _sparse_position(), _hash_eval
    ref = R.search(cells, player, n_moves, S, C_PUCT, evalf)
    s = B.search(cells, player, n_moves, S, 1, C_PUCT, evalf)
    t = s.t
    assert t.W == ref.W and t.visits == ref.visits  # float64, bit for bit
    assert t.parent == ref.parent and t.move == ref.move and t.term == ref.term
    assert t.cells == ref.cells and t.value == ref.value  # the same nodes in the same order
    assert [p for p in t.prior] == [p for p in ref.prior]
    assert s.terminal_sims == 0 and s.rounds == S + 1 and s.collisions == 0 and s.batch_terminals == 0
    assert s.rows_active == s.n_evals == sum(1 for x in ref.term if x == 0)


# ---------------------------------------------------------------- 2. invariants at K > 1
def _snapshot(t):
    return (list(t.W), list(t.visits), list(t.parent), list(t.move), list(t.term), list(t.value), list(t.cells),
            [None if p is None else list(p) for p in t.prior])


@pytest.mark.parametrize("S,K", [(7, 2), (7, 4), (7, 8), (24, 2), (24, 4), (24, 8), (3, 8)])
@pytest.mark.parametrize("case", ["tactical_uniform", "sparse_hash"])
def test_batched_search_invariants(S, K, case):
    if case == "tactical_uniform":
        (cells, player, n_moves), evalf = R.tactical_position(), R.uniform_eval
    else:
        (cells, player, n_moves), evalf = _sparse_position(), _hash_eval
    s = B.search(cells, player, n_moves, S, K, C_PUCT, evalf)
    t = s.t
    assert t.visits[0] == S + 1 and s.remaining() == 0
    assert sum(t.root_visits()) == S
    assert len(t.parent) <= S + 1
    # (no simulation of these cases ends in a terminal node; one that does takes no row,
    # test_open_four_backs_up_terminals_inside_a_batch)
    assert s.terminal_sims == 0 and 1 + -(-S // K) <= s.rounds <= S + 1
    assert t.visits == s.through  # every node's visits = the backups through it
    assert s.n_evals == sum(1 for x in t.term if x == 0) == s.rows_active
    assert all(p is not None for p, x in zip(t.prior, t.term) if x == 0)  # no node is left unevaluated
    before, counters = _snapshot(t), (s.rounds, s.collisions, s.batch_terminals, s.n_evals)
    for _ in range(3):  # a game at its budget has only inactive rows: extra rounds change nothing
        assert s.round() == [None] * K
    assert _snapshot(t) == before and (s.rounds, s.collisions, s.batch_terminals, s.n_evals) == counters


# ---------------------------------------------------------------- 3. collisions, terminals in a batch
def test_peaked_prior_collides_in_round_one():
    cells, player, n_moves = _sparse_position()
    cell = 100
    assert cells[cell] == 0
    S, K = 24, 4
    evalf = B.peaked_eval(cell)
    s = B.Search(cells, player, n_moves, S, K, C_PUCT, evalf)
    assert s.round() == [tuple(cells), None, None, None]
    # the second descent of round 1 picks the child under `cell` again: at the root
    # -1 + u / 2 beats every other cell's exploration term
    pr = s.t.prior[0]
    u = ((C_PUCT * pr[cell]) * 2.0 ** 0.5) / 2.0
    others = max(((C_PUCT * pr[c]) * 2.0 ** 0.5) / 1.0 for c in range(225) if cells[c] == 0 and c != cell)
    assert -1.0 + u > others
    rows = s.round()
    assert s.collisions == 1 and rows[0] is not None and rows[1:] == [None, None, None]
    assert rows[0][cell] == player and s.t.visits[0] == 2
    while s.remaining() > 0:
        s.round()
    assert s.collisions >= 1 and s.rounds > 1 + -(-S // K)  # the collisions cost rounds
    assert s.t.visits[0] == S + 1 and sum(s.t.root_visits()) == S and s.t.visits == s.through
    assert s.rows_active < s.rows_total


def test_open_four_backs_up_terminals_inside_a_batch():
    cells, player, n_moves = R.tactical_position()
    win = 7 * 15 + 7
    S, K = 24, 4
    s = B.Search(cells, player, n_moves, S, K, C_PUCT, B.boosted_eval(win))
    s.round()
    rows = s.round()
    # round 1: the first descent creates the five (a terminal child, backed up at once, no
    # row); its W is +1 per visit, so every later descent revisits it.  A simulation that
    # ends in a terminal node takes no row: the whole budget fits into this one round
    assert s.t.move[1] == win and s.t.term[1] == player and rows == [None] * K
    assert s.batch_terminals == S - 1 and s.terminal_sims == S and s.t.visits[1] == S
    assert s.remaining() == 0 and s.rounds == 2 and len(s.t.parent) == 2
    assert s.t.visits == s.through and sum(s.t.root_visits()) == S
    # one leaf per round orders the same simulations the same way
    one = B.search(cells, player, n_moves, S, 1, C_PUCT, B.boosted_eval(win))
    assert (one.t.W, one.t.visits, one.t.move) == (s.t.W, s.t.visits, s.t.move)


def test_blocked_four_mixes_leaves_and_terminals_in_a_batch():
    # white's first tries are (6,10) and the block at (7,7); under (6,10) black's boosted
    # reply at (7,7) is the five: a terminal grandchild, created and followed inside a batch
    cells, player, n_moves = B.blocked_four()
    S, K = 24, 4
    evalf = B.boosted_eval((100, 112))
    s = B.search(cells, player, n_moves, S, K, C_PUCT, evalf, extra_rounds=2)
    t = s.t
    assert s.batch_terminals >= 1 and 0 < s.terminal_sims < S
    assert any(x == 1 for x in t.term) and s.n_evals >= 2
    assert t.visits[0] == S + 1 and sum(t.root_visits()) == S and t.visits == s.through
    assert len(t.parent) <= S + 1
    assert 1 + -(-(S - s.terminal_sims) // K) <= s.rounds <= S + 1


# ---------------------------------------------------------------- 4. the library without a GPU
def _batch_params(K, S=16, flags=None):
    flags = _lib.GZ_PUCT_LEAF_BATCH if flags is None else flags
    return _lib.PuctBatchParams(S, 0, C_PUCT, 0, _lib.GZ_PV_F16X3, flags, 0.0, 0.0, K, 0)


@pytest.mark.parametrize("K", [0, 33, -1])
def test_leaves_per_round_out_of_range_is_an_argument_error(K):
    L = _lib.load()
    p = _batch_params(K)
    # (non-NULL pointers would be needed only after the argument checks; none is touched)
    args = (None, None, 1, ctypes.cast(ctypes.byref(p), ctypes.POINTER(_lib.PuctParams)), None, None, None, None, None,
            None)
    assert L.gz_puct_search(*args) == -1 and b"leaves_per_round" in L.gz_last_error()
    assert L.gz_puct_begin(None, None, 1, args[3], None, None, None, None) == -1
    assert b"leaves_per_round" in L.gz_last_error()
    assert L.gz_selfplay_puct_run(None, 1, args[3], None, None, 1, None, 0, None, None, None) == -1
    assert b"leaves_per_round" in L.gz_last_error()
    # without the flag nothing past the 32 bytes is read: the same struct passes this check
    q = _batch_params(K, flags=0)
    assert L.gz_puct_search(None, None, 1, ctypes.cast(ctypes.byref(q), ctypes.POINTER(_lib.PuctParams)), None, None,
                            None, None, None, None) == -1
    assert b"leaves_per_round" not in L.gz_last_error()


def test_tree_reuse_rejects_a_batched_configuration():
    L = _lib.load()
    p = _batch_params(4)
    pp = ctypes.cast(ctypes.byref(p), ctypes.POINTER(_lib.PuctParams))
    one = ctypes.c_int64(0)
    ptr = ctypes.addressof(one)  # any non-NULL pointers: the check comes before every GPU call
    assert L.gz_selfplay_puct_rounds(ptr, 1, pp, ptr, ptr, 1, ptr, 0, ptr, ptr, None) == -1
    assert b"leaves_per_round > 1" in L.gz_last_error()


def test_batch_sizes_and_surface():
    L = _lib.load()
    assert ctypes.sizeof(_lib.PuctBatchParams) == 56 and _lib.PuctBatchParams.leaves_per_round.offset == 48
    assert _lib.GZ_PUCT_LEAF_BATCH == 2 and _lib.GZ_PUCT_MAX_LEAVES == 32
    for n, S in ((1, 16), (5, 24), (64, 200)):
        assert L.gz_puct_batch_workspace_bytes(n, S, 1) >= L.gz_puct_workspace_bytes(n, S)
        assert L.gz_selfplay_puct_batch_workspace_bytes(n, S, 1) >= L.gz_selfplay_puct_workspace_bytes(n, S)
        sizes = [L.gz_puct_batch_workspace_bytes(n, S, K) for K in (1, 2, 4, 8, 32)]
        assert sizes == sorted(sizes) and sizes[-1] > sizes[0]
        # the round buffers grow by at least leaves, prior, probs, logits, value and active per row
        assert sizes[3] - sizes[0] >= n * 7 * (64 + 1800 + 900 + 900 + 4 + 4)


def test_python_parameter_checks():
    from gzero import device
    p = device.puct_params(16, C_PUCT)
    assert type(p) is _lib.PuctParams and p.flags == 0  # the default: today's struct, the flag clear
    assert device.puct_leaves(p) == 0
    b = device.puct_params(16, C_PUCT, leaves_per_round=4)
    assert type(b) is _lib.PuctBatchParams and b.flags == _lib.GZ_PUCT_LEAF_BATCH and b.leaves_per_round == 4
    nb = device.puct_params(16, C_PUCT, dirichlet_alpha=0.3, leaves_per_round=8)
    assert nb.flags == 3 and nb.noise_alpha == 0.3 and nb.leaves_per_round == 8 and device.puct_leaves(nb) == 8
    assert device.with_leaves(p, None) is p and device.with_leaves(p, 1) is p
    w = device.with_leaves(nb, 2)
    assert w.leaves_per_round == 2 and w.flags == 3 and w.noise_eps == nb.noise_eps and w.seed == nb.seed
    for bad in (0, 33):
        with pytest.raises(ValueError):
            device.puct_params(16, C_PUCT, leaves_per_round=bad)
    from ai_agent import AlphaZeroGomokuAI
    from gzero.selfplay import SelfPlayEngine
    with pytest.raises(ValueError):
        AlphaZeroGomokuAI(1, leaves_per_round=4)  # search="reference"
    with pytest.raises(ValueError):
        SelfPlayEngine(n_slots=4, leaves_per_round=4)
    with pytest.raises(ValueError):
        SelfPlayEngine(n_slots=4, search="puct", tree_reuse=True, leaves_per_round=4, pv_weights=object())
