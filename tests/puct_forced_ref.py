"""Plain-Python restatement of forced playouts and policy-target pruning in the PUCT search
(GZ_PUCT_FORCED_PLAYOUTS: include/gzero.h, csrc/gz_forced.h, csrc/gz_puct.hip), on top of
tests/puct_ref.py, tests/puct_reuse_ref.py, tests/puct_noise_ref.py and tests/puct_cap_ref.py.
The checker of tests/test_puct_forced_cpu.py and tests/test_gpu_puct_forced.py.  Not a test.

Every float is a Python float (IEEE binary64) and every operation is written in the order
the header performs it, so trees and rows compare with ``==``.

Forcing: at the root of a search whose budget is the full one (B == S), a child with
n >= 1 visits scores +infinity while n < sqrt((k * prior[0][c]) * (visits[0] - 1)).
Pruning: the visit row that leaves such a root gives back, child by child, the forced
playouts the child would not hold by PUCT against the most-visited child's score.  The move
is chosen from the raw counts and the tree keeps them.
"""
import math

import puct_cap_ref as CR
import puct_ref as R
import puct_reuse_ref as RR

CELLS = R.CELLS
INF = float("inf")


class Counters:
    """Per search (or per game): simulations whose root selection went to a cell with a
    forced (infinite) score, and visits taken out of rows by prune_row."""

    def __init__(self):
        self.forced_selections = 0
        self.pruned_visits = 0


def forced_min(k, prior, T):
    return math.sqrt((k * prior) * float(T))


def simulate(t, c_puct, evalf, k, counters=None):
    """puct_reuse_ref.simulate with the forcing at the root (k = 0: none)."""
    i = 0
    while True:
        if t.term[i]:
            t.backup(i, 0.0 if t.term[i] == 3 else -1.0)
            return
        board, prior = t.cells[i], t.prior[i]
        sq = math.sqrt(float(t.visits[i]))
        best, bc = None, -1
        for c in range(CELLS):
            if board[c] != 0:
                continue
            j = t.child[i].get(c)
            n = t.visits[j] if j is not None else 0
            q = t.W[j] / n if n else 0.0
            u = ((c_puct * prior[c]) * sq) / (1.0 + n)
            score = q + u
            if i == 0 and j is not None and n >= 1 and float(n) < forced_min(k, prior[c], t.visits[0] - 1):
                score = INF
            if best is None or score > best:
                best, bc = score, c
        if i == 0 and best == INF and counters is not None:
            counters.forced_selections += 1
        j = t.child[i].get(bc)
        if j is not None:
            i = j
            continue
        mover, count = t.player[i], t.count[i] + 1
        nb = list(board)
        nb[bc] = mover
        if R.makes_five(nb, bc, mover):
            term = mover
        elif 0 not in nb or count >= 200:
            term = 3
        else:
            term = 0
        j = t.add(i, bc, term, nb, 3 - mover, count)
        t.child[i][bc] = j
        if term:
            t.backup(j, 0.0 if term == 3 else -1.0)
        else:
            t.prior[j], v = evalf(t.cells[j], 3 - mover)
            t.value[j] = v
            t.backup(j, v)
        return


def prune_counts(c_puct, k, N, prior, W, visits):
    """The pruned row of one root: N = visits[0], and per cell the root row's prior, the
    child's W and its visits (0: no child).  A new list."""
    out = list(visits)
    best_c, best_n = -1, 0
    for c in range(CELLS):
        if visits[c] > best_n:
            best_c, best_n = c, visits[c]
    if best_c < 0:
        return out
    sq = math.sqrt(float(N))
    best = W[best_c] / float(best_n) + ((c_puct * prior[best_c]) * sq) / (1.0 + float(best_n))
    for c in range(CELLS):
        n = visits[c]
        if c == best_c or n < 1:
            continue
        q = W[c] / float(n)
        m = min(n, int(forced_min(k, prior[c], N - 1)))
        r = 0
        while r < m:
            s = q + ((c_puct * prior[c]) * sq) / (1.0 + float(n - (r + 1)))
            if s >= best:
                break
            r += 1
        out[c] = n - r
        if r > 0 and out[c] == 1:
            out[c] = 0
    return out


def prune_row(t, c_puct, k, counters=None):
    """The visit row tree t hands out at a full-budget root."""
    raw = t.root_visits()
    W = [0.0] * CELLS
    for c, j in t.child[0].items():
        W[c] = t.W[j]
    prior = t.prior[0] if t.prior[0] is not None else [0.0] * CELLS
    out = prune_counts(c_puct, k, t.visits[0], prior, W, raw)
    if counters is not None:
        counters.pruned_visits += sum(raw) - sum(out)
    return out


def search(cells, player, n_moves, S, c_puct, evalf, k, noise=None, counters=None):
    """puct_ref.search (with the noise of puct_noise_ref when given) and the forcing: the
    tree after S simulations.  The row to hand out is prune_row(tree, c_puct, k)."""
    t = RR.fresh(cells, player, n_moves, evalf)
    if noise is not None:
        noise.mix_root(t)
    for _ in range(S):
        simulate(t, c_puct, evalf, k, counters)
    return t


def play_game(seed, game_id, S, c_puct, temp_plies, evalf, k, noise=None, reuse=True, F=None, full_prob=1.0,
              max_plies=200, on_ply=None, counters=None):
    """One self-play game from the empty board.  reuse: the own-clock engine (the subtree
    under the move is the next tree), else the lock-step one (a fresh root every ply).
    F: the playout cap (None: every ply is full); a ply whose budget is not S neither
    forces nor prunes.  Returns (moves, visit rows as handed out, raw visit rows, z per
    ply, full flag per ply); on_ply(ply, tree before the move)."""
    cap = F is not None

    def kind(ply):
        full = CR.is_full(seed, game_id, ply, full_prob) if cap else True
        return full, (S if full else F)

    full, B = kind(0)
    t = CR.evaluate(RR.fresh([0] * CELLS, 1, 0), evalf, full, noise)
    moves, rows, raws, fulls = [], [], [], []
    winner, over = 0, False
    while not over and len(moves) < max_plies:
        kk = k if B == S else 0.0
        while t.visits[0] < B + 1:
            simulate(t, c_puct, evalf, kk, counters)
        mv, _ = R.choose_move(t, temp_plies, seed, game_id)
        moves.append(mv)
        raws.append(t.root_visits())
        rows.append(prune_row(t, c_puct, k, counters) if B == S else t.root_visits())
        fulls.append(full)
        if on_ply:
            on_ply(len(moves) - 1, t)
        mover = t.player[0]
        j = t.child[0].get(mv)
        nfull, nB = kind(len(moves))
        if reuse:
            nt, over = RR.advance(t, mv)
            if noise is not None and nfull and not over and nt.prior[0] is not None:
                noise.mix_root(nt)
        elif j is not None and t.term[j]:
            nt, over = None, True
        else:
            nt, over = RR.fresh(t.cells[j], t.player[j], t.count[j]), False
        if over:
            won = t.term[j] != 3 if j is not None else R.makes_five(nt.cells[0], mv, mover)
            winner = mover if won else 0
            break
        t, B, full = nt, nB, nfull
        if t.prior[0] is None:
            CR.evaluate(t, evalf, full, noise)
    z = [0 if winner == 0 else (1 if 1 + p % 2 == winner else -1) for p in range(len(moves))]
    return moves, rows, raws, z, fulls
