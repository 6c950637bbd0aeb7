"""Plain-Python restatement of playout cap randomization in the PUCT search
(GZ_PUCT_PLAYOUT_CAP: include/gzero.h, csrc/gz_puct.hip), on top of tests/puct_ref.py,
tests/puct_reuse_ref.py and tests/puct_noise_ref.py.  The checker of
tests/test_puct_cap_cpu.py and tests/test_gpu_puct_cap.py.  Not a test.

Every ply of a game is full or fast, a pure function of (seed, game id, ply):

    full = to_unit(draw(stream_key(seed, game, ply, CAP_SIM), 0)) < full_prob

The budget B of the root at that ply is S when full, else F.  It is decided when the
node becomes a root and a search is finished when visits[0] >= B + 1.  An inherited
root that arrives with v >= B + 1 visits gets no simulation; its visit row is the
inherited child visits as they are (summing to v - 1) and its move takes one round.
Every other row sums to B; a move takes B + 1 rounds on a fresh root and B + 1 - v on an
inherited one.  Root noise (a puct_noise_ref.Noise) is mixed into the roots of full
plies only, at the two places of puct_noise_ref: the backup of a fresh root's
evaluation, and right after the re-root for an inherited one.
"""
import puct_ref as R
import puct_reuse_ref as RR
from gzero import rng

CELLS = R.CELLS
CAP_SIM = 0x50434150  # "PCAP"


def is_full(seed, game_id, ply, full_prob):
    return rng.to_unit(rng.draw(rng.stream_key(seed, game_id, ply, CAP_SIM), 0)) < full_prob


def budget(seed, game_id, ply, S, F, full_prob):
    return S if is_full(seed, game_id, ply, full_prob) else F


def remaining(t, B, over=False):
    """gz_puct_remaining / gz_puct_reroot's d_remaining for tree t with the budget B."""
    return 0 if over else max(0, B + 1 - t.visits[0])


def evaluate(t, evalf, full, noise=None):
    """The backup of a one-node root that waits for its evaluation (one round); the
    noise is mixed in on a full ply."""
    assert t.prior[0] is None and len(t.parent) == 1
    t.prior[0], v = evalf(t.cells[0], t.player[0])
    t.value[0] = v
    t.backup(0, v)
    if noise is not None and full:
        noise.mix_root(t)
    return t


def advance(t, move, seed, game_id, S, F, full_prob, noise=None):
    """The tree after `move` at t's root: (tree, over, B, full) with the budget of the new
    ply.  An inherited live root of a full ply is mixed at once; a fresh root (a move
    without a child) waits for evaluate()."""
    nt, over = RR.advance(t, move)
    full = is_full(seed, game_id, nt.count[0], full_prob)
    if noise is not None and full and not over and nt.prior[0] is not None:
        noise.mix_root(nt)
    return nt, over, (S if full else F), full


def play_game(seed, game_id, S, F, full_prob, c_puct, temp_plies, evalf, noise=None, max_plies=200, on_ply=None,
              force=None):
    """One self-play game from the empty board with tree reuse and the playout cap.
    Returns (moves, visit rows, z per ply, rounds per move, full flag per ply).
    on_ply(ply, tree before the move, tree after the re-root / the fresh root or None,
    info) with info = dict(full, budget, inherited: the visits the root arrived with or
    None for a fresh root, remaining: the count after the move).  force(ply, tree) may
    return a move to play instead of the chosen one (None: the chosen one)."""
    full = is_full(seed, game_id, 0, full_prob)
    B = S if full else F
    t = evaluate(RR.fresh([0] * CELLS, 1, 0), evalf, full, noise)
    rounds, inherited = 1, None
    moves, rows, per_move, fulls = [], [], [], []
    winner, over = 0, False
    while not over and len(moves) < max_plies:
        while t.visits[0] < B + 1:
            RR.simulate(t, c_puct, evalf)
            rounds += 1
        mv = force(len(moves), t) if force is not None else None
        if mv is None:
            mv, _ = R.choose_move(t, temp_plies, seed, game_id)
        moves.append(mv)
        rows.append(t.root_visits())
        per_move.append(max(rounds, 1))
        fulls.append(full)
        info = {"full": full, "budget": B, "inherited": inherited}
        mover = t.player[0]
        nt, over, nB, nfull = advance(t, mv, seed, game_id, S, F, full_prob, noise)
        if over:
            j = t.child[0].get(mv)
            won = t.term[j] != 3 if j is not None else R.makes_five(nt.cells[0], mv, mover)
            winner = mover if won else 0
        info["remaining"] = remaining(nt, nB, over)
        if on_ply:
            on_ply(len(moves) - 1, t, nt, info)
        if over:
            break
        t, B, full = nt, nB, nfull
        if t.prior[0] is None:  # a fresh root: its evaluation is the first round
            evaluate(t, evalf, full, noise)
            rounds, inherited = 1, None
        else:
            rounds, inherited = 0, t.visits[0]
    z = [0 if winner == 0 else (1 if 1 + k % 2 == winner else -1) for k in range(len(moves))]
    return moves, rows, z, per_move, fulls
