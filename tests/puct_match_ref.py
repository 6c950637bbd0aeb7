"""The PUCT arena restated in plain Python (gz_puct_match_run / gz_puct_match_results,
include/gzero.h): which side moves, the tally of a match's records, the Wilson interval,
and a driver that plays the games ply by ply from Python -- per ply one gz_puct_search
per side over the live games that side moves in.  The forward's rows are bit-identical
whatever the batch (tests/test_gpu_pv_edges.py), so the driver is exact."""
import math

import numpy as np

import puct_ref as R

TALLY_FIELDS = ("games", "a_wins", "b_wins", "draws", "a_wins_black", "a_wins_white", "b_wins_black",
                "b_wins_white", "plies")


def side_of(game_id, player, parity):
    """0 (side A) or 1 (side B): A plays black (player 1) in game g iff ((g ^ parity) & 1) == 0."""
    a_black = ((int(game_id) ^ int(parity)) & 1) == 0
    return 0 if (player == 1) == a_black else 1


def tally(records, parity):
    """The tally of records (anything with game_id, ply, z per row): a game counts once,
    at its ply-0 record, whose mover is black and whose z is black's result."""
    t = dict.fromkeys(TALLY_FIELDS, 0)
    result = {}
    for r in records:
        t["plies"] += 1
        if int(r["ply"]) != 0:
            continue
        a_black = side_of(r["game_id"], 1, parity) == 0
        res = int(r["z"]) if a_black else -int(r["z"])
        result[int(r["game_id"])] = res
        t["games"] += 1
        if res > 0:
            t["a_wins"] += 1
            t["a_wins_black" if a_black else "a_wins_white"] += 1
        elif res < 0:
            t["b_wins"] += 1
            t["b_wins_white" if a_black else "b_wins_black"] += 1
        else:
            t["draws"] += 1
    return t, result


def wilson(score, n, z=1.959963984540054):
    """Wilson score interval of score / n."""
    p = score / n
    denom = 1.0 + z * z / n
    centre = p + z * z / (2 * n)
    spread = z * math.sqrt((p * (1 - p) + z * z / (4 * n)) / n)
    return ((centre - spread) / denom, (centre + spread) / denom)


def drive(games, sides, p, parity=0, max_plies=200):
    """Play the games (ids) to the end, or for max_plies plies.  sides: the two PVWeights (A,
    B); p: puct_params keywords without the precision (num_simulations, c_puct, temp_plies,
    seed, dirichlet_alpha, noise_eps).  Returns {id: dict(moves, visits [plies][225], z per
    ply, winner 0/1/2, over, cells per ply after the move)}."""
    from gzero import boards, device
    params = [device.puct_params(precision=w.precision, **p) for w in sides]
    out = {int(g): {"moves": [], "visits": [], "after": [], "winner": 0, "over": False} for g in games}
    cells = {g: [0] * 225 for g in out}
    for k in range(max_plies):
        live = [g for g in out if not out[g]["over"]]
        if not live:
            break
        player = 1 + k % 2
        for sd in (0, 1):
            mine = [g for g in live if side_of(g, player, parity) == sd]
            if not mine:
                continue
            states = np.concatenate([boards.make_states(np.array(cells[g], np.int8)[None], n_moves=k, player=player)
                                     for g in mine])
            mv, vis, _, _ = device.puct_search(states, mine, params[sd], sides[sd])
            for i, g in enumerate(mine):
                m = int(mv[i])
                assert 0 <= m < 225 and cells[g][m] == 0, (g, k, m)
                cells[g][m] = player
                o = out[g]
                o["moves"].append(m)
                o["visits"].append(vis[i].copy())
                o["after"].append(tuple(cells[g]))
                if R.makes_five(cells[g], m, player):
                    o["over"], o["winner"] = True, player
                elif 0 not in cells[g] or k + 1 >= 200:
                    o["over"] = True
    for o in out.values():
        w = o["winner"]
        o["z"] = [0 if (w == 0 or not o["over"]) else (1 if 1 + k % 2 == w else -1) for k in range(len(o["moves"]))]
    return out
