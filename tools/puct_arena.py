#!/usr/bin/env python3
"""The PUCT arena (gzero.arena.PuctMatch, gz_puct_match_run) measured and recorded.

a. The cost of the routed round: one match step (one ply of every game: S+1 rounds of
   select, gather, two forwards, scatter, backup) at --games x --sims, f16x3 on both sides
   with the same blob, against the lock-step self-play step of tools/puct_bench.py's
   --lockstep-child, which loads --lockstep-library (a build of the parent commit) if
   given.  Both stand at the same positions (the same seed, 24 burn-in plies at 8
   simulations: with one blob on both sides a match plays the self-play games) and take
   turns at one step each, --steps times, timed with device events.
b. The wall time of a whole match of --games games with compaction.
c. Two recorded matches with their Wilson intervals: the same blob on both sides (the
   first-move advantage, in the colour split; this is also the match of b) and f16
   against f16x3 on the same init weights.

    python tools/puct_arena.py --lockstep-library parent/libgzero.so --out profiles/puct/match_bench.json
"""
import argparse
import json
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "alphazero-gomoku_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--games", type=int, default=4096)
ap.add_argument("--sims", type=int, default=200)
ap.add_argument("--burn", type=int, default=24, help="burn-in plies of the step measurement (8 simulations each)")
ap.add_argument("--steps", type=int, default=5)
ap.add_argument("--temp-plies", type=int, default=12)
ap.add_argument("--seed", type=int, default=1)
ap.add_argument("--lockstep-library", default=None, help="libgzero.so the self-play child loads (the parent commit's)")
ap.add_argument("--skip-matches", action="store_true", help="only the step measurement")
ap.add_argument("--note", default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


# the child first, while this process has not opened the GPU
env = dict(os.environ)
if a.lockstep_library:
    env["GZ_LIBRARY"] = os.path.abspath(a.lockstep_library)
child = subprocess.Popen([sys.executable, os.path.join(REPO, "tools", "puct_bench.py"), "--lockstep-child", "1.0",
                          "--slots", str(a.games), "--sims", str(a.sims), "--burn", str(a.burn), "--precisions",
                          "f16x3", "--temp-plies", str(a.temp_plies)], env=env, stdin=subprocess.PIPE,
                         stdout=subprocess.PIPE, text=True)
try:
    if child.stdout.readline().strip() != "READY":
        sys.exit(f"self-play child failed ({child.poll()})")
    import torch
    from gzero import arena, device, weights
    blob = weights.pack_pv_weights(weights.init_state_dict(0))
    w3, w1 = device.PVWeights(blob, "f16x3"), device.PVWeights(blob, "f16")
    kw = dict(num_simulations=a.sims, temp_plies=a.temp_plies, seed=a.seed)
    m = arena.PuctMatch(w3, w3, a.games, compact=False, **kw)
    m.advance(a.burn)
    m.step()  # warm-up at the timed shape, as the child's
    torch.cuda.synchronize()
    match_ms, self_ms, match_moves = [], [], []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        m.launch(1)
        e1.record()
        torch.cuda.synchronize()
        match_moves.append(int(m.counters()["moves"]))  # (below --games: slots whose game ended in the burn-in idle)
        match_ms.append(e0.elapsed_time(e1))
        child.stdin.write("step\n")
        child.stdin.flush()
        line = child.stdout.readline().split()
        if len(line) != 2 or line[0] != "STEP_MS":
            sys.exit(f"self-play child failed ({child.poll()}): {line}")
        self_ms.append(float(line[1]))
finally:
    child.stdin.close()
    child.wait(timeout=120)
del m
torch.cuda.empty_cache()
rounds = a.sims + 1
step = {"match_step_ms": match_ms, "selfplay_step_ms": self_ms, "match_moves_per_step": match_moves,
        "selfplay_moves_per_step": a.games, "match_step_ms_median": median(match_ms),
        "selfplay_step_ms_median": median(self_ms), "match_round_ms": median(match_ms) / rounds,
        "selfplay_round_ms": median(self_ms) / rounds, "match_over_selfplay": median(match_ms) / median(self_ms),
        "target": 1.10, "extra_bytes_per_round": a.games * (64 + 1800 + 4)}
print(f"step: match {step['match_step_ms_median']:.1f} ms, self-play {step['selfplay_step_ms_median']:.1f} ms "
      f"(x{step['match_over_selfplay']:.4f}; round {step['match_round_ms']:.4f} / {step['selfplay_round_ms']:.4f} ms)",
      flush=True)
res = {"config": {"games": a.games, "simulations": a.sims, "temp_plies": a.temp_plies, "seed": a.seed,
                  "burn_in_plies": a.burn, "steps": a.steps, "weights": "init_state_dict(0) on both sides",
                  "timing": "device events around one step (one ply of every game, S+1 rounds); the match in this "
                            "process and the lock-step self-play step in a child process take turns",
                  "selfplay_library": "another build (--lockstep-library)" if a.lockstep_library else "this build"},
       "device": torch.cuda.get_device_name(0), "step": step, "matches": {}}
if a.note:
    res["config"]["note"] = a.note


def recorded(name, wa, wb):
    t0 = time.perf_counter()
    mt = arena.PuctMatch(wa, wb, a.games, **kw)
    out = arena.summarise(mt.run())
    torch.cuda.synchronize()
    out["seconds"] = time.perf_counter() - t0
    out.update(a=wa.precision, b=wb.precision, steps=mt.steps, moves_played=mt.moves_played)
    res["matches"][name] = out
    print(f"{name}: {out['wins']} / {out['losses']} / {out['draws']} (A {wa.precision} wins / B {wb.precision} wins "
          f"/ draws), A as black {out['wins_black']} won {out['losses_black']} lost, as white {out['wins_white']} won "
          f"{out['losses_white']} lost; score {out['score']:.4f}, 95 % Wilson [{out['wilson95'][0]:.4f}, "
          f"{out['wilson95'][1]:.4f}]; {out['plies']} plies in {out['seconds']:.1f} s", flush=True)
    del mt
    torch.cuda.empty_cache()


if not a.skip_matches:
    recorded("same_blob_f16x3", w3, w3)
    recorded("f16_against_f16x3", w1, w3)
    res["whole_match_seconds"] = res["matches"]["same_blob_f16x3"]["seconds"]
print("PUCT_ARENA_JSON " + json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
