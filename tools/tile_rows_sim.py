#!/usr/bin/env python3
"""Executed MFMA rows of pv_dg_kernel's tap-skipping gather for 16-row tiles
(v_mfma_f32_16x16x32_f16, shipped) and 32-row tiles (v_mfma_f32_32x32x16_f16, VERDICT r05
item 2b), simulated on the kernel's own row classification (csrc/gz_pvdg.hip dg_rows_all):
rows of a pass = the on-board positions of its nodes' output squares, counting-sorted by the
class (ty-set, tx-set) in the kernel's rank order (csrc/gz_dgclass.h dg_class_rank), cut into
tiles, each tile running the union of its rows' taps.  Chunks: 6 children of a random root
with stones on consecutive empty cells in descending row-major order (the search expands the
highest empty cell first, ai_agent.py:224-249).  Prints executed tile-taps x rows per child
for the shipped class order and, for comparison, the round-6 one (--seed: another sample)."""
import argparse

import numpy as np

BN = 15
SETS = (1, 3, 7, 6, 4, 2)  # the 6 tap sets of an axis (bit 0: -1, bit 1: 0, bit 2: +1)
GROUP = {0: 6, 1: 3, 2: 2, 3: 1}  # nodes per pass of layer L

# round 6: axis order {-1,0,1},{-1,0},{-1},{0,1},{0},{1}, class = rank(ty) * 6 + rank(tx)
_R06 = {7: 0, 3: 1, 1: 2, 6: 3, 2: 4, 4: 5}
# shipped: the nested axis order {-1},{-1,0},{-1,0,1},{0,1},{1},{0} (each set beside its
# supersets), the x order reversed on odd y ranks (a snake: neighbouring classes differ on
# one axis only)
_NEST = {1: 0, 3: 1, 7: 2, 6: 3, 4: 4, 2: 5}


def rank_r06(ty, tx):
    return _R06[ty] * 6 + _R06[tx]


def rank_nested_snake(ty, tx):
    ry, rx = _NEST[ty], _NEST[tx]
    return ry * 6 + (5 - rx if ry & 1 else rx)


ORDERS = {"r06": rank_r06, "nested-snake": rank_nested_snake}
SHIPPED = "nested-snake"


def pass_rows(cells, L, rank=rank_nested_snake):
    RO, RIN = L + 2, L + 1
    rows = []
    for cell in cells:
        cr, cc = divmod(cell, BN)
        for dy in range(-RO, RO + 1):
            for dx in range(-RO, RO + 1):
                pr, pc = cr + dy, cc + dx
                if not (0 <= pr < BN and 0 <= pc < BN):
                    continue
                ty = tx = 0
                for d in (-1, 0, 1):
                    qy, qx = dy + d, dx + d
                    if -RIN <= qy <= RIN and 0 <= cr + qy < BN:
                        ty |= 1 << (d + 1)
                    if -RIN <= qx <= RIN and 0 <= cc + qx < BN:
                        tx |= 1 << (d + 1)
                if not ty or not tx:
                    continue
                taps = {(a, b) for a in range(3) if ty >> a & 1 for b in range(3) if tx >> b & 1}
                rows.append((rank(ty, tx), taps))
    rows.sort(key=lambda r: r[0])
    return rows


def tile_taps(rows, T):
    n = 0
    for i in range(0, len(rows), T):
        u = set()
        for _, t in rows[i:i + T]:
            u |= t
        n += len(u)
    return n


def sample_chunks(seed=1, n=400):
    """the tool's sample: n chunks of 6 children of random roots"""
    rng = np.random.default_rng(seed)
    chunks = []
    for _ in range(n):
        ns = int(rng.integers(4, 80))
        occ = set(rng.choice(225, size=ns, replace=False).tolist())
        empty = [c for c in range(224, -1, -1) if c not in occ]
        s = int(rng.integers(0, len(empty) - 6))
        chunks.append(empty[s:s + 6])
    return chunks


def simulate(rank, chunks):
    """executed tile-taps of the chunks under a class order: (children, ideal row-taps,
    {tile rows: tile-taps x rows}, 16-row tile-taps per layer)"""
    tot = {16: 0, 32: 0}
    layer = [0, 0, 0, 0]
    row_taps = 0
    for chunk in chunks:
        for L in range(4):
            g = GROUP[L]
            for k in range(0, 6, g):
                rows = pass_rows(chunk[k:k + g], L, rank)
                row_taps += sum(len(t) for _, t in rows)
                for T in (16, 32):
                    tot[T] += tile_taps(rows, T) * T
                layer[L] += tile_taps(rows, 16)
    return 6 * len(chunks), row_taps, tot, layer


def tile_taps_per_child(rank, seed=1):
    kids, _, tot, _ = simulate(rank, sample_chunks(seed))
    return tot[16] / 16 / kids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    chunks = sample_chunks(a.seed)
    for name in (SHIPPED, "r06"):
        kids, row_taps, tot, layer = simulate(ORDERS[name], chunks)
        print(f"{name}{' (shipped)' if name == SHIPPED else ''}: per child: ideal row-taps {row_taps / kids:.0f}; "
              f"executed rows x taps: 16-row tiles {tot[16] / kids:.0f} ({tot[16] / 16 / kids:.1f} tile-taps; "
              f"y1 / x1 / y2 / x2 {' / '.join(f'{x / kids:.1f}' for x in layer)}), 32-row tiles {tot[32] / kids:.0f} "
              f"(+{(tot[32] / tot[16] - 1) * 100:.1f} % MFMA work)")


if __name__ == "__main__":
    main()
