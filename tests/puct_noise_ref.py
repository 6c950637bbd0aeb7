"""Plain-Python restatement of the Dirichlet noise at the PUCT search root
(csrc/gz_dirichlet.h, the GZ_PUCT_ROOT_NOISE paths of csrc/gz_puct.hip), on top of
tests/puct_ref.py and tests/puct_reuse_ref.py.  The checker of
tests/test_puct_noise_cpu.py and tests/test_gpu_puct_noise.py.  Not a test.

Every float is a Python float (IEEE binary64) and every operation is written in the
order the header performs it, with frexp, ldexp, floor and sqrt of ``math``, so
samples and mixed rows compare with ``==``.

A root's prior row is mixed exactly once: when its evaluation is backed up (a fresh
root) or right after the re-root that made it the root (an inherited one), with the
stream of (seed, game id, the root's move count, NOISE_SIM).
"""
import math

import puct_ref as R
import puct_reuse_ref as RR
from gzero import rng

CELLS = R.CELLS
NOISE_SIM = 0x4E4F4953
DRAWS = 256

LN2_HI = float.fromhex("0x1.62e42fee00000p-1")
LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
INV_LN2 = float.fromhex("0x1.71547652b82fep+0")
SQRT_HALF = float.fromhex("0x1.6a09e667f3bcdp-1")
FACT = [float(math.factorial(d)) for d in range(14)]


def unit(x):
    return ((x >> 11) + 1) * (1.0 / 9007199254740992.0)


def gz_log(x):
    m, e = math.frexp(x)
    if m < SQRT_HALF:
        m = m * 2.0
        e -= 1
    s = (m - 1.0) / (m + 1.0)
    z = s * s
    p = 1.0 / 23.0
    for k in range(21, 0, -2):
        p = p * z + 1.0 / k
    e = float(e)
    return (e * LN2_HI + (2.0 * s) * p) + e * LN2_LO


def gz_exp(x):
    if x < -708.0:
        return 0.0
    k = math.floor(x * INV_LN2 + 0.5)
    kf = float(k)
    r = (x - kf * LN2_HI) - kf * LN2_LO
    p = 1.0 / FACT[13]
    for d in range(12, -1, -1):
        p = p * r + 1.0 / FACT[d]
    return math.ldexp(p, k)


def gamma_cell(key, c, alpha, used=None):
    """Gamma(alpha) of cell c; used (a list) receives the largest draw index read."""
    base = DRAWS * c
    d = (alpha + 1.0) - 1.0 / 3.0
    cc = 1.0 / math.sqrt(9.0 * d)
    i = 1
    while True:
        if i + 3 > DRAWS:
            return 0.0
        a = 2.0 * unit(rng.draw(key, base + i)) - 1.0
        b = 2.0 * unit(rng.draw(key, base + i + 1)) - 1.0
        u = unit(rng.draw(key, base + i + 2))
        i += 3
        s = a * a + b * b
        if s >= 1.0 or s == 0.0:
            continue
        x = a * math.sqrt((-2.0 * gz_log(s)) / s)
        t = 1.0 + cc * x
        if t <= 0.0:
            continue
        v = (t * t) * t
        if gz_log(u) < (((0.5 * x) * x + d) - d * v) + d * gz_log(v):
            break
    if used is not None:
        used.append(i - 1)
    return (d * v) * gz_exp(gz_log(unit(rng.draw(key, base))) / alpha)


def noise_key(seed, game_id, ply):
    return rng.stream_key(seed, game_id, ply, NOISE_SIM)


def eta(seed, game_id, ply, empty, alpha):
    """eta[225] (0.0 at stones) or None when the total is 0 or not finite; empty: 225
    truth values."""
    key = noise_key(seed, game_id, ply)
    g = [gamma_cell(key, c, alpha) if empty[c] else 0.0 for c in range(CELLS)]
    total = 0.0
    for c in range(CELLS):
        if empty[c]:
            total += g[c]
    if not (total > 0.0 and math.isfinite(total)):
        return None
    return [g[c] / total if empty[c] else 0.0 for c in range(CELLS)]


def eta_row(seed, game_id, ply, empty, alpha):
    """eta as gz_puct_root_noise stores it: an all-zero row in place of None."""
    e = eta(seed, game_id, ply, empty, alpha)
    return [0.0] * CELLS if e is None else e


def mix(prior, cells, seed, game_id, ply, alpha, eps):
    """The mixed row (a new list); stones keep the evaluator's entry."""
    empty = [x == 0 for x in cells]
    e = eta(seed, game_id, ply, empty, alpha)
    if e is None:
        return list(prior)
    return [(1.0 - eps) * prior[c] + eps * e[c] if empty[c] else prior[c] for c in range(CELLS)]


class Noise:
    def __init__(self, seed, game_id, alpha, eps):
        self.seed, self.game_id, self.alpha, self.eps = seed, game_id, alpha, eps

    def mix_root(self, t):
        """Mix the root row of tree t in place (the root must be evaluated and live)."""
        t.prior[0] = mix(t.prior[0], t.cells[0], self.seed, self.game_id, t.count[0], self.alpha, self.eps)


def fresh(cells, player, n_moves, evalf, noise):
    """puct_reuse_ref.fresh with an evaluated root whose row is mixed at its backup."""
    t = RR.fresh(cells, player, n_moves, evalf)
    noise.mix_root(t)
    return t


def search(cells, player, n_moves, S, c_puct, evalf, noise):
    """puct_ref.search with the noise at the root: the root's evaluation, the mix, then
    S simulations."""
    t = fresh(cells, player, n_moves, evalf, noise)
    for _ in range(S):
        RR.simulate(t, c_puct, evalf)
    return t


def advance(t, move, noise):
    """puct_reuse_ref.advance with the noise: (tree, over).  An inherited live root is
    mixed at once with the key of its new ply; a fresh root waits for its evaluation
    (evaluate() mixes it); a terminal root has no row to mix."""
    nt, over = RR.advance(t, move)
    if not over and nt.prior[0] is not None:
        noise.mix_root(nt)
    return nt, over


def evaluate(t, evalf, noise):
    """The backup of a fresh root that waited for its evaluation (advance's move
    without a child)."""
    assert t.prior[0] is None and len(t.parent) == 1
    t.prior[0], v = evalf(t.cells[0], t.player[0])
    t.value[0] = v
    t.backup(0, v)
    noise.mix_root(t)
    return t
