"""Plain-Python restatement of PUCT tree reuse between plies (csrc/gz_puct.hip:
puct_reroot_kernel, gz_selfplay_puct_rounds), on top of tests/puct_ref.py.  The
checker of tests/test_puct_reuse_cpu.py and tests/test_gpu_puct_reuse.py.  Not a test.

A search is a root evaluation (``fresh``) and then simulations (``simulate``, the body
of ``puct_ref.search``'s loop) until the root has S+1 visits, the state in which a
fresh search ends.  ``reroot(tree, j)`` is the tree of the next ply: the subtree of
node j, nodes kept in creation order and renumbered densely, every per-node value
carried as it is.  A round is one step of a game's clock: the root evaluation, or one
simulation (whether or not it ends in an evaluation).
"""
import math

import puct_ref as R

CELLS = R.CELLS


def fresh(cells, player, n_moves, evalf=None):
    """A one-node tree; with evalf the root is evaluated (one round), without it the
    root waits for its evaluation (visits 0)."""
    t = R.Tree()
    t.add(-1, 255, 0, cells, player, n_moves)
    if evalf is not None:
        t.prior[0], v = evalf(t.cells[0], player)
        t.value[0] = v
        t.backup(0, v)
    return t


def simulate(t, c_puct, evalf):
    """One simulation of puct_ref.search on tree t (in place)."""
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
            if best is None or score > best:
                best, bc = score, c
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


def reroot(t, j):
    """The subtree of node j (>= 1) as a tree of its own."""
    n = len(t.parent)
    new = {}
    for k in range(n):  # parents precede children
        if k == j or t.parent[k] in new:
            new[k] = len(new)
    out = R.Tree()
    for k in sorted(new):
        out.parent.append(-1 if k == j else new[t.parent[k]])
        out.move.append(255 if k == j else t.move[k])
        out.term.append(t.term[k])
        out.visits.append(t.visits[k])
        out.W.append(t.W[k])
        out.child.append({c: new[x] for c, x in t.child[k].items()})
        out.prior.append(t.prior[k])
        out.value.append(t.value[k])
        out.cells.append(t.cells[k])
        out.player.append(t.player[k])
        out.count.append(t.count[k])
    return out


def depth_of(t, k):
    d = 0
    while t.parent[k] >= 0:
        k = t.parent[k]
        d += 1
    return d


def advance(t, move):
    """The tree after `move` is played at t's root: (tree, over).  A chosen child that
    is terminal ends the game (its one node is kept, nothing else); a move without a
    child gives a fresh root that waits for its evaluation."""
    j = t.child[0].get(move)
    if j is not None:
        nt = reroot(t, j)
        return nt, nt.term[0] != 0
    mover, count = t.player[0], t.count[0] + 1
    nb = list(t.cells[0])
    assert nb[move] == 0
    nb[move] = mover
    over = R.makes_five(nb, move, mover) or 0 not in nb or count >= 200
    return fresh(nb, 3 - mover, count), over


def play_game(seed, game_id, S, c_puct, temp_plies, evalf, reuse=True, max_plies=200, on_ply=None):
    """One self-play game from the empty board.  Returns (moves, visit rows, z per ply,
    rounds per move); on_ply(ply, tree before the move, tree after re-rooting or None)."""
    t = fresh([0] * CELLS, 1, 0, evalf)
    rounds = 1
    moves, rows, per_move = [], [], []
    winner, over = 0, False
    while not over and len(moves) < max_plies:
        while t.visits[0] < S + 1:
            simulate(t, c_puct, evalf)
            rounds += 1
        mv, _ = R.choose_move(t, temp_plies, seed, game_id)
        moves.append(mv)
        rows.append(t.root_visits())
        per_move.append(rounds)
        rounds = 0
        j = t.child[0][mv]
        nt = None
        if t.term[j]:
            over, winner = True, (0 if t.term[j] == 3 else t.term[j])
        elif reuse:
            nt = reroot(t, j)
        else:
            nt = fresh(t.cells[j], t.player[j], t.count[j], evalf)
            rounds = 1
        if on_ply:
            on_ply(len(moves) - 1, t, nt if reuse else None)
        t = nt
    z = [0 if winner == 0 else (1 if 1 + k % 2 == winner else -1) for k in range(len(moves))]
    return moves, rows, z, per_move
