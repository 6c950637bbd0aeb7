"""Plain-Python restatement of the Gumbel root with sequential halving (csrc/gz_gumbel.h, the
GZ_PUCT_GUMBEL paths of csrc/gz_puct.hip; Danihelka et al., ICLR 2022), on top of
tests/puct_ref.py and tests/puct_noise_ref.py (gz_log, gz_exp, unit).  The checker of
tests/test_puct_gumbel_cpu.py and tests/test_gpu_puct_gumbel.py.  Not a test.

Every float is a Python float (IEEE binary64) and every operation is written in the order
the header performs it, so scores, rows and trees compare with ``==``.
"""
import math
import sys

import puct_noise_ref as NR
import puct_ref as R
from gzero import rng

CELLS = R.CELLS
GUMBEL_SIM = 0x47554D42
MAX_CONSIDERED = 32
ROW_SCALE = 32767.0
DBL_MIN = sys.float_info.min
DBL_MAX = sys.float_info.max
NEG_INF = -math.inf


def seq(m, S):
    """The considered-visits sequence of sequential halving."""
    if m <= 1:
        return list(range(S))
    L = (m - 1).bit_length()  # ceil(log2 m)
    visits = [0] * m
    k = m
    out = []
    while len(out) < S:
        x = max(1, S // (L * k))
        for _ in range(x):
            out += visits[:k]
            for i in range(k):
                visits[i] += 1
        k = max(2, k // 2)
    return out[:S]


def prior_ok(p):
    return DBL_MIN <= p <= DBL_MAX  # (a NaN fails)


def ok_cells(prior, empty):
    """(ok[225], any_ok): the empty cells whose prior has a logarithm, or every empty cell."""
    any_ok = any(empty[c] and prior_ok(prior[c]) for c in range(CELLS))
    return [bool(empty[c]) and (not any_ok or prior_ok(prior[c])) for c in range(CELLS)], any_ok


def logit(p, any_ok):
    return NR.gz_log(p) if any_ok else 0.0


def gumbel(key, c, gumbel_scale):
    u = NR.unit(rng.draw(key, c))
    e = -NR.gz_log(u)
    if not e >= DBL_MIN:
        e = float.fromhex("0x1p-53")
    return gumbel_scale * (-NR.gz_log(e))


def gumbel_key(seed, game_id, ply):
    return rng.stream_key(seed, game_id, ply, GUMBEL_SIM)


def base_row(seed, game_id, ply, prior, empty, gumbel_scale):
    """(base[225] with None at the cells that are not ok, ok[225])."""
    ok, any_ok = ok_cells(prior, empty)
    key = gumbel_key(seed, game_id, ply)
    return [gumbel(key, c, gumbel_scale) + logit(prior[c], any_ok) if ok[c] else None for c in range(CELLS)], ok


def root(seed, game_id, ply, prior, empty, max_considered, gumbel_scale):
    """(gs[225], the considered cells in the order they were taken)."""
    base, ok = base_row(seed, game_id, ply, prior, empty, gumbel_scale)
    m = min(max_considered, sum(ok))
    gs = [NEG_INF] * CELLS
    taken = []
    for _ in range(m):
        bc = -1
        for c in range(CELLS):
            if ok[c] and c not in taken and (bc < 0 or base[c] > base[bc]):
                bc = c
        taken.append(bc)
        gs[bc] = base[bc]
    return gs, taken


def sigma(c_visit, c_scale, maxN, q):
    return ((c_visit + float(maxN)) * c_scale) * q


def score(gs, c_visit, c_scale, maxN, want, W, n):
    if want == 0:
        return gs
    return gs + sigma(c_visit, c_scale, maxN, W / float(n))


def policy(prior, empty, W, visits, v0, c_visit, c_scale):
    """(pi[225], row[225]) from the root's row, its empty cells and, per cell, W and the visits
    of its child (0: none)."""
    ok, any_ok = ok_cells(prior, empty)
    sumN, maxN = 0, 0
    P = A = 0.0
    for c in range(CELLS):
        n = visits[c]
        if n < 1:
            continue
        sumN += n
        maxN = max(maxN, n)
        P += prior[c]
        A += prior[c] * (W[c] / float(n))
    v_mix = (v0 + float(sumN) * (A / P)) / (1.0 + float(sumN)) if (sumN > 0 and P > 0.0) else v0
    x = [0.0] * CELLS
    mx = None
    for c in range(CELLS):
        if not ok[c]:
            continue
        cq = W[c] / float(visits[c]) if visits[c] >= 1 else v_mix
        x[c] = logit(prior[c], any_ok) + sigma(c_visit, c_scale, maxN, cq)
        if mx is None or x[c] > mx:
            mx = x[c]
    Z = 0.0
    for c in range(CELLS):
        if ok[c]:
            x[c] = NR.gz_exp(x[c] - mx)
            Z += x[c]
    pi = [x[c] / Z if ok[c] else 0.0 for c in range(CELLS)]
    return pi, [int(pi[c] * ROW_SCALE + 0.5) if ok[c] else 0 for c in range(CELLS)]


class Gumbel:
    def __init__(self, seed, game_id, max_considered=16, c_visit=50.0, c_scale=0.5, gumbel_scale=1.0):
        self.seed, self.game_id = seed, game_id
        self.max_considered, self.c_visit, self.c_scale, self.gumbel_scale = max_considered, c_visit, c_scale, gumbel_scale


def prepare(t, gm):
    """Root preparation of tree t, whose root has just been evaluated: t.gs, t.considered."""
    empty = [x == 0 for x in t.cells[0]]
    t.gs, t.considered = root(gm.seed, gm.game_id, t.count[0], t.prior[0], empty, gm.max_considered, gm.gumbel_scale)


def child_stats(t):
    """(visits[225], W[225]) of the root's children, 0 / 0.0 where there is none."""
    v, w = [0] * CELLS, [0.0] * CELLS
    for c, j in t.child[0].items():
        v[c], w[c] = t.visits[j], t.W[j]
    return v, w


def root_cell(t, gm, S):
    """The root's cell of simulation visits[0] - 1."""
    v, w = child_stats(t)
    want = seq(len(t.considered), S)[t.visits[0] - 1]
    maxN = max(v)
    best, bc = None, -1
    for c in range(CELLS):
        if t.gs[c] == NEG_INF or v[c] != want:
            continue
        sc = score(t.gs[c], gm.c_visit, gm.c_scale, maxN, want, w[c], v[c])
        if best is None or sc > best:
            best, bc = sc, c
    assert bc >= 0, "by construction there is always a candidate"
    return bc


def select(t, c_puct, first):
    """One descent with the root's cell given and PUCT below the root (puct_reuse_ref.simulate's
    loop): the new node that waits for its evaluation, or None when a terminal node was backed
    up."""
    i = 0
    while True:
        if t.term[i]:
            t.backup(i, 0.0 if t.term[i] == 3 else -1.0)
            return None
        board, prior = t.cells[i], t.prior[i]
        if i == 0:
            bc = first
        else:
            sq = math.sqrt(float(t.visits[i]))
            best, bc = None, -1
            for c in range(CELLS):
                if board[c] != 0:
                    continue
                j = t.child[i].get(c)
                n = t.visits[j] if j is not None else 0
                q = t.W[j] / n if n else 0.0
                u = ((c_puct * prior[c]) * sq) / (1.0 + n)
                sc = q + u
                if best is None or sc > best:
                    best, bc = sc, c
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
            return None
        return j


def receive(t, j, prior, v, gm):
    """Node j's evaluation: stored, backed up and, for the root, the root preparation."""
    t.prior[j] = prior
    t.value[j] = v
    t.backup(j, v)
    if j == 0:
        prepare(t, gm)


def new_tree(cells, player, n_moves):
    """A one-node tree whose root waits for its evaluation."""
    t = R.Tree()
    t.add(-1, 255, 0, cells, player, n_moves)
    return t


def simulate(t, c_puct, evalf, gm, S):
    """One round after the root's: the schedule's cell, the descent, the evaluation."""
    j = select(t, c_puct, root_cell(t, gm, S))
    if j is not None:
        prior, v = evalf(t.cells[j], t.player[j])
        receive(t, j, prior, v, gm)


def begin(cells, player, n_moves, evalf, gm):
    """The tree after the root's round: evaluated, backed up, prepared."""
    t = new_tree(cells, player, n_moves)
    prior, v = evalf(t.cells[0], player)
    receive(t, 0, prior, v, gm)
    return t


def search(cells, player, n_moves, S, c_puct, evalf, gm):
    """The tree after S simulations from a live position."""
    t = begin(cells, player, n_moves, evalf, gm)
    for _ in range(S):
        simulate(t, c_puct, evalf, gm, S)
    return t


def choose_move(t, gm):
    """The move: among the considered cells with the most visits the first maximum of
    gs + sigma(q); no draw."""
    v, w = child_stats(t)
    maxN = max(v)
    cmax = max(v[c] for c in t.considered)
    best, bc = None, -1
    for c in range(CELLS):
        if t.gs[c] == NEG_INF or v[c] != cmax:
            continue
        sc = score(t.gs[c], gm.c_visit, gm.c_scale, maxN, cmax, w[c], v[c])
        if best is None or sc > best:
            best, bc = sc, c
    return bc


def target(t, gm):
    """(pi, row) that leave the search."""
    v, w = child_stats(t)
    return policy(t.prior[0], [x == 0 for x in t.cells[0]], w, v, t.value[0], gm.c_visit, gm.c_scale)
