"""Plain-Python restatement of leaf batching with virtual loss in the PUCT search
(GZ_PUCT_LEAF_BATCH; puct_select_batch_kernel and puct_backup_batch_kernel of
csrc/gz_puct.hip), on top of tests/puct_ref.py.  The checker of
tests/test_puct_batch_cpu.py and tests/test_gpu_puct_batch.py.  Not a test.

Every float is a Python float (IEEE binary64) and every operation is written in the
order the kernels perform it, so trees compare with ``==``.

A search is finished when ``visits[0] == S + 1``.  Round 0 evaluates the root alone (row
0 of the game's K rows).  In every later round the game descends up to K times, one
descent after the other; ``vl[x]`` counts the leaves of this round that wait below node
``x`` -- zero at the start of the round, never kept past it -- and enters the score as
that many visits, each lost by the selector (a node's ``W`` is from the view of the
player who moved into it, the selector at its parent):

    n = visits[j] + vl[j];  q = (W[j] - vl[j]) / n if n else 0.0
    score = q + ((c_puct * prior[i][c]) * sqrt(visits[i] + vl[i])) / (1.0 + n)

so K = 1 is puct_ref.search bit for bit (``W - 0.0``, ``n + 0``).  A descent starts only
while ``visits[0] + vl[0] <= S`` (finished + in-flight simulations); one that reaches a
terminal node backs up at once and takes no row; one that selects a node created in this
round and not yet evaluated (a collision) changes nothing and ends the game's selection
for the round; any other creates a node, whose board is the game's next row.  The backup
step then evaluates the rows in ascending order.
"""
import math

import puct_ref as R

CELLS = R.CELLS


class Search:
    """One game's batched search, driven round by round.

    ``rows = s.round()`` runs one round (select unless it is round 0, then the evaluation
    and backup of its rows) and returns the K rows of the round: the cells tuple of an
    active row, None for an inactive one.  Counters: ``rounds`` (rounds that began with
    the search unfinished), ``collisions``, ``batch_terminals`` (terminal backups that a
    later descent of the same round follows: the tree words the select kernel writes and
    reads back in one launch), ``terminal_sims`` (simulations that ended in a terminal
    node: they take no row, so a round completes up to K leaves plus any number of them,
    and a move takes between 1 + ceil((S - terminal_sims) / K) and S + 1 rounds),
    ``n_evals``, ``rows_active`` / ``rows_total`` (over the
    counted rounds), ``through[x]`` (backups that passed through node x)."""

    def __init__(self, cells, player, n_moves, S, K, c_puct, evalf, noise=None):
        self.S, self.K, self.c_puct, self.evalf, self.noise = S, K, c_puct, evalf, noise
        self.t = R.Tree()
        self.t.add(-1, 255, 0, cells, player, n_moves)
        self.through = [0]
        self.pend = [0]  # round 0: the root, in row 0
        self.calls = 0
        self.rounds = self.collisions = self.batch_terminals = self.terminal_sims = self.n_evals = 0
        self.rows_active = self.rows_total = 0

    def remaining(self):
        return self.S + 1 - self.t.visits[0]

    def _backup(self, i, v):
        self.t.backup(i, v)
        while i >= 0:
            self.through[i] += 1
            i = self.t.parent[i]

    def _select(self):
        t, S, K, c_puct = self.t, self.S, self.K, self.c_puct
        vl = [0] * (S + 2)
        first = len(t.parent)
        pend = []
        waiting = 0  # terminal backups of this round that no later descent has followed yet
        while len(pend) < K and t.visits[0] + vl[0] <= S:
            self.batch_terminals += waiting
            waiting = 0
            i, path = 0, [0]
            stop = False
            while True:
                if t.term[i]:
                    self._backup(i, 0.0 if t.term[i] == 3 else -1.0)
                    self.terminal_sims += 1
                    waiting += 1
                    break
                board, prior = t.cells[i], t.prior[i]
                sq = math.sqrt(float(t.visits[i] + vl[i]))
                best, bc = None, -1
                for c in range(CELLS):
                    if board[c] != 0:
                        continue
                    j = t.child[i].get(c)
                    n = t.visits[j] + vl[j] if j is not None else 0
                    q = (t.W[j] - float(vl[j])) / float(n) if n else 0.0
                    score = q + ((c_puct * prior[c]) * sq) / (1.0 + float(n))
                    if best is None or score > best:
                        best, bc = score, c
                j = t.child[i].get(bc)
                if j is not None:
                    if j >= first and t.term[j] == 0:  # created in this round, not yet evaluated
                        self.collisions += 1
                        stop = True
                        break
                    i = j
                    path.append(j)
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
                self.through.append(0)
                t.child[i][bc] = j
                if term:
                    self._backup(j, 0.0 if term == 3 else -1.0)
                    self.terminal_sims += 1
                    waiting += 1
                else:
                    pend.append(j)
                    for x in path + [j]:
                        vl[x] += 1
                break
            if stop:
                break
        self.pend = pend

    def begin_round(self):
        """The select step (none in round 0): the K rows of the round."""
        self.counted = self.remaining() > 0
        if self.calls:
            self._select()
        self.calls += 1
        return [self.t.cells[j] for j in self.pend] + [None] * (self.K - len(self.pend))

    def end_round(self, results):
        """The backup step: results = (prior, value) of the active rows, in row order."""
        t = self.t
        assert len(results) == len(self.pend)
        for j, (prior, v) in zip(self.pend, results):  # ascending rows
            t.prior[j] = prior
            if j == 0 and self.noise is not None:
                self.noise.mix_root(t)
            t.value[j] = v
            self._backup(j, v)
            self.n_evals += 1
        if self.counted:
            self.rounds += 1
            self.rows_active += len(self.pend)
            self.rows_total += self.K
        self.pend = []

    def round(self):
        rows = self.begin_round()
        self.end_round([self.evalf(self.t.cells[j], self.t.player[j]) for j in self.pend])
        return rows


def search(cells, player, n_moves, S, K, c_puct, evalf, noise=None, extra_rounds=0):
    """The finished Search of a live position (``.t`` is its tree), then extra_rounds more
    rounds, which must change nothing."""
    s = Search(cells, player, n_moves, S, K, c_puct, evalf, noise)
    while s.remaining() > 0:
        s.round()
    for _ in range(extra_rounds):
        rows = s.round()
        assert rows == [None] * K
    return s


def peaked_eval(cell, mass=0.999):
    """evalf: `mass` of the prior on `cell` while it is empty, the rest spread evenly
    over the other empty cells; value 0.0.  With K >= 2 the second descent of round 1
    collides at the root: the child under `cell` has q = -1 and half the exploration
    term, -1 + u / 2, which still beats every other cell's u."""

    def evalf(cells, player):
        empty = [c for c in range(CELLS) if cells[c] == 0]
        prior = [0.0] * CELLS
        if cells[cell] != 0 or len(empty) == 1:
            for c in empty:
                prior[c] = 1.0 / len(empty)
        else:
            for c in empty:
                prior[c] = mass if c == cell else (1.0 - mass) / (len(empty) - 1)
        return prior, 0.0

    return evalf


def boosted_eval(boost, weight=50.0):
    """evalf: the uniform prior with `weight` times the share at the cells of `boost` (a
    cell or several); value 0.0.  On puct_ref.tactical_position() with one of black's two
    winning cells boosted, the first descent of round 1 creates the terminal child and
    the later ones of that round revisit it (its W is +1 per visit): terminal backups
    inside a batch."""
    boost = (boost,) if isinstance(boost, int) else tuple(boost)

    def evalf(cells, player):
        w = [0.0 if x else 1.0 for x in cells]
        for c in boost:
            if cells[c] == 0:
                w[c] = weight
        total = math.fsum(w)
        return [x / total for x in w], 0.0

    return evalf


def blocked_four():
    """puct_ref.tactical_position() with one more black stone and white to move: whatever
    white plays, black completes the five at (7,2) or (7,7).  (cells, player, n_moves)"""
    cells, _, _ = R.tactical_position()
    cells[16] = 1
    return cells, 2, 9
