"""Plain-Python restatement of the PUCT search mode (csrc/gz_puct.hip), the
checker of tests/test_puct_cpu.py and tests/test_gpu_puct.py.  Not a test.

``v`` is the value for the side to move at node ``i``; a node's ``W`` is from the
view of the player who moved into it.  Every float is a Python float (IEEE
binary64) and every operation is written in the order the kernel performs it, so
trees compare with ``==``.

``evalf(cells, player) -> (prior, value)``: ``cells`` a tuple of 225 ints (0 empty,
1 black, 2 white), ``player`` the side to move; ``prior`` 225 floats (only the
entries at empty cells are read), ``value`` a float (the kernel's
``(double)float32``).
"""
import math

from gzero import rng

N = 15
CELLS = 225
DIRS = ((0, 1), (1, 0), (1, 1), (1, -1))


def makes_five(cells, c, player):
    """check_win (gomoku_board.py): a run of five or more through cell c, already placed."""
    r0, c0 = divmod(c, N)
    for dr, dc in DIRS:
        run = 1
        for sg in (1, -1):
            r, q = r0 + sg * dr, c0 + sg * dc
            while 0 <= r < N and 0 <= q < N and cells[r * N + q] == player:
                run += 1
                r, q = r + sg * dr, q + sg * dc
        if run >= 5:
            return True
    return False


class Tree:
    def __init__(self):
        self.parent, self.move, self.term, self.visits, self.W = [], [], [], [], []
        self.child, self.prior, self.value, self.cells, self.player, self.count = [], [], [], [], [], []

    def add(self, parent, move, term, cells, player, count):
        self.parent.append(parent)
        self.move.append(move)
        self.term.append(term)
        self.visits.append(0)
        self.W.append(0.0)
        self.child.append({})
        self.prior.append(None)
        self.value.append(0.0)
        self.cells.append(tuple(cells))
        self.player.append(player)
        self.count.append(count)
        return len(self.parent) - 1

    def backup(self, i, v):
        s = -v
        while i >= 0:
            self.visits[i] += 1
            self.W[i] += s
            s = -s
            i = self.parent[i]

    def root_visits(self):
        out = [0] * CELLS
        for c, j in self.child[0].items():
            out[c] = self.visits[j]
        return out


def search(cells, player, n_moves, S, c_puct, evalf):
    """The tree after S simulations from a live position."""
    t = Tree()
    t.add(-1, 255, 0, cells, player, n_moves)
    t.prior[0], v = evalf(t.cells[0], player)
    t.value[0] = v
    t.backup(0, v)
    for _ in range(S):
        i = 0
        while True:
            if t.term[i]:
                t.backup(i, 0.0 if t.term[i] == 3 else -1.0)
                break
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
            if makes_five(nb, bc, mover):
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
            break
    return t


def choose_move(tree, temp_plies, seed, game_id):
    """(move, main-stream draws) from the root visit counts."""
    visits = tree.root_visits()
    board, n_moves = tree.cells[0], tree.count[0]
    total = sum(visits)
    if n_moves >= temp_plies or total == 0:
        best, bc = -2, -1
        for c in range(CELLS):
            x = visits[c] if board[c] == 0 else -1
            if x > best:
                best, bc = x, c
        return bc, 0
    pick = (rng.draw(rng.stream_key(seed, game_id, n_moves, 0), 0) * total) >> 64
    run = 0
    for c in range(CELLS):
        run += visits[c]
        if run > pick:
            return c, 1
    raise AssertionError("pick < total")


def root_q(tree):
    return -tree.W[0] / tree.visits[0]


def uniform_eval(cells, player):
    k = cells.count(0)
    return [1.0 / k if x == 0 else 0.0 for x in cells], 0.0


def tactical_position():
    """Black (7,3)..(7,6), white at the corners, black to move, 8 moves played."""
    cells = [0] * CELLS
    for c in (7 * N + 3, 7 * N + 4, 7 * N + 5, 7 * N + 6):
        cells[c] = 1
    for c in (0, 14, 210, 224):
        cells[c] = 2
    return cells, 1, 8
