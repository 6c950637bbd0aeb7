#!/usr/bin/env python3
"""Self-play rate of the PUCT search mode (SelfPlayEngine(search="puct")).

For each precision: n_slots games are brought to a mix of positions (burn-in plies
at 8 simulations), then `--steps` one-ply steps of gz_selfplay_puct_run are timed
with device events (moves/s = slots / median step time).  One more search of the
same boards is driven round by round through the step API with events around
select, forward and backup, for the per-round times.  The standalone gz_pv_forward
of n_slots boards is timed in a child process, which loads --forward-library (a
build of another commit, e.g. the parent's) if given: (S+1) x that time is what the
forwards alone cost, the rest of a step is the search kernels and launch gaps.

    python tools/puct_bench.py --out profiles/puct/bench.json

--reuse measures tree reuse between plies (SelfPlayEngine(tree_reuse=True)) instead:
after the burn-in and a warm-up of 4 x (S+1) rounds (the slots' clocks drift apart),
three windows of 2 x (S+1) rounds are timed with device events: ms per round, the moves
played in the window, mean rounds per move (the rounds those moves took, from the slot
statistics; slots that stay in phase play a whole number of moves per window, so slots
x rounds / moves is quantised) and moves/s = slots / (rounds per move x ms per round).  The
lock-step step is timed in the same call, alternating with the windows, in a child
process (its own engine, same slots, simulations, burn-in and weights) that loads
--lockstep-library (GZ_LIBRARY: a build of the parent commit) if given.  The init
weights give a nearly flat prior, so runs with the policy FC scaled by
--policy-scale are added: a synthetic, sharper prior that shows how the reuse depends on
how peaked the search is -- not a trained network.

    python tools/puct_bench.py --reuse --lockstep-library parent/libgzero.so \\
        --out profiles/puct/reuse_bench.json

--noise ALPHA,EPS measures the Dirichlet noise at the search root
(SelfPlayEngine(dirichlet_alpha=ALPHA, noise_eps=EPS)): three child processes, each with
its own engine (same slots, simulations, burn-in and weights) -- this build with the
noise, this build without it, and --lockstep-library (a build of the parent commit)
without it -- take turns at one timed lock-step step each, --steps times; with --reuse
the same again with tree-reuse engines and windows of 2 x (S+1) rounds.  Then the effect
the noise exists for: the distinct positions among the slots after --distinct-plies
plies from the empty board at temp_plies 0 (play without noise is deterministic there),
noise on and off.

    python tools/puct_bench.py --noise 0.3,0.25 --reuse --precisions f16x3 --steps 5 \\
        --lockstep-library parent/libgzero.so --out profiles/puct/noise_bench.json

--gumbel M measures the Gumbel root with sequential halving
(SelfPlayEngine(gumbel_considered=M), lock-step): a round of the parent build
(--lockstep-library), of this build with the flag clear and with it set, child processes
taking turns; the select / forward / backup / finish launches of a step-API search with and
without the flag (device events); moves/s at the budgets of --gumbel-sims, measured on a
lock-step engine and as the arithmetic slots / ((S + 1) x round); and the mean
KL(pi' || prior) of the rows recorded by --gumbel-kl-slots games at --gumbel-kl-sims
simulations, at the init weights and with the policy FC scaled (--policy-scale).  No claim
about playing strength.

    python tools/puct_bench.py --gumbel 16 --precisions f16x3 --steps 7 \\
        --lockstep-library parent/libgzero.so --out profiles/puct/gumbel_bench.json

--forced K measures forced playouts and policy-target pruning
(SelfPlayEngine(forced_playouts=K)) the way --noise measures the noise, with the root noise
of --forced-noise on in all three engines: the parent build (--lockstep-library), this build
with the flag clear and with it set take turns as child processes, lock-step and (--reuse)
own-clock.  Then what the feature does, from gz_puct_search on --forced-positions mid-game
positions with that noise, flag clear and set under the same seed: the share of a full
search's visits the forcing threshold covers and the share it displaced, the share pruned
from the rows, and the target mass on the cells whose noised prior exceeds twice the clean
one -- at the init weights and with the policy FC scaled by --policy-scale (synthetic nets with
a favourite move).

    python tools/puct_bench.py --forced 2 --reuse --precisions f16x3 --steps 5 \\
        --lockstep-library parent/libgzero.so --out profiles/puct/forced_bench.json

--sym measures the leaf symmetry (SelfPlayEngine(leaf_symmetry=True)) the way --noise
measures the noise: three child processes -- the parent build, this build with the flag
clear, this build with the flag set -- take turns at one timed step each, lock-step and
with --reuse; then the orientation dependence of the search (orientation_dependence).

    python tools/puct_bench.py --sym --reuse --precision f16x3 --steps 5 \\
        --lockstep-library parent/libgzero.so --out profiles/puct/sym_bench.json

--leaves K,K,... measures leaf batching with virtual loss (SelfPlayEngine(leaves_per_round=K))
at small slot counts: for every count of --sweep-slots two child processes -- this build with
one engine per K, and --lockstep-library (a build of the parent commit, which has no K > 1: the
K = 1 baseline) -- take turns at one timed lock-step step (one move per slot) each, --steps
times, with device events.  Before a timed step the child drives the same boards once more
through the step API, untimed, and counts what the step will run: the rounds (with the block
rule of gz_puct_search: 1 + ceil(S/K), then ceil(left/K) until nothing is left), the host
reads and the active rows.  Reported per (slots, K): ms per move (= per step), rounds per
move, ms per round and the share of forward rows that were empty (collisions, the budget's
tail, round 0's K - 1 unused rows per game).

    python tools/puct_bench.py --leaves 1,2,4,8,16 --precisions f16x3 --steps 5 \\
        --lockstep-library parent/libgzero.so --out profiles/puct/batch_bench.json

--compact measures slot compaction (training.selfplay_puct_device(compact=True)): one
self-play iteration of G games on G slots, for every G of --compact-games, without root
noise and with --compact-noise.  Three child processes -- this build compacting, this build
with continuous refill (compact=False) and --lockstep-library (a build of the parent commit)
with continuous refill -- take turns at one whole iteration each, --steps times; reported per
child: seconds per iteration (wall clock around the call, median of the turns), steps, moves
played, the mean and longest game and the device time of the compaction launches themselves.
mean / longest game is the ratio the forward's row count alone predicts for seconds with
compaction / without.  Then the path with compaction off: one lock-step step at --slots
against the parent build, as --leaves 1 measures it.

    python tools/puct_bench.py --compact --precisions f16x3 --steps 3 \\
        --lockstep-library parent/libgzero.so --out profiles/puct/compact_bench.json

--cap F,P measures playout cap randomization (SelfPlayEngine(tree_reuse=True,
fast_simulations=F, full_prob=P)) on the own-clock engine, for the init weights and for
every --policy-scale: two engines of this build in one process (same slots, simulations,
burn-in, seed and weights), without the cap -- the path of before, the baseline -- and with
it, take turns at one window of 2 x (S+1) rounds each, --steps times, after the warm-up of
--reuse.  Per engine: ms per round (median, and every window: the baseline's spread), the
moves played, mean rounds per move (slot statistics) and moves/s = slots / (rounds per move
x ms per round).  Then one training.selfplay_puct_device iteration of --cap-games games on
as many slots each way (wall clock, after one untimed iteration that warms the allocator):
seconds, plies, and full-ply records; from the capped iteration's whole games the share of
full plies and of plies that needed no new simulation (the root arrived with at least its
budget + 1 visits: the previous row's count at the move played).

    python tools/puct_bench.py --cap 40,0.25 --precisions f16x3 --out profiles/puct/cap_bench.json

--precision f16x3|f16|fp32 runs the lock-step, --reuse or --leaves measurement at that one
precision (it replaces --precisions).  "f16" is the one-term fp16 tower (GZ_PV_F16); a child
that loads another build (--forward-library, --lockstep-library: the parent commit, which
has no f16) runs f16x3 instead, so every f16 figure stands beside the parent's f16x3 of the
same call.

    python tools/puct_bench.py --precision f16 --forward-library parent/libgzero.so
    python tools/puct_bench.py --reuse --precision f16 --lockstep-library parent/libgzero.so
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "alphazero-gomoku_amd"))

ap = argparse.ArgumentParser()
ap.add_argument("--slots", type=int, default=4096)
ap.add_argument("--sims", type=int, default=200)
ap.add_argument("--burn", type=int, default=24, help="burn-in plies (8 simulations each)")
ap.add_argument("--steps", type=int, default=3)
ap.add_argument("--precisions", default="f16x3,fp32")
ap.add_argument("--precision", default=None, choices=["f16x3", "f16", "fp32"],
                help="the one precision of the lock-step, --reuse or --leaves measurement (replaces --precisions)")
ap.add_argument("--temp-plies", type=int, default=12)
ap.add_argument("--forward-library", default=None, help="libgzero.so the standalone forward is timed on")
ap.add_argument("--forward-only", action="store_true", help="(child) time gz_pv_forward alone, print JSON")
ap.add_argument("--note", default=None, help="free text stored in the result's config (e.g. which build --forward-library is)")
ap.add_argument("--reuse", action="store_true", help="measure tree reuse between plies (see above)")
ap.add_argument("--policy-scale", default="32,128",
                help="--reuse, --cap, --forced: the policy FC's weight and bias times this in the synthetic runs (comma-separated)")
ap.add_argument("--lockstep-library", default=None, help="--reuse: libgzero.so the lock-step child loads")
ap.add_argument("--lockstep-child", type=float, default=None, metavar="SCALE",
                help="(child) time lock-step steps on request, policy FC scaled by SCALE")
ap.add_argument("--noise", default=None, metavar="ALPHA,EPS", help="measure the root noise (see above)")
ap.add_argument("--distinct-plies", type=int, default=8, help="--noise: plies of the distinct-positions count")
ap.add_argument("--noise-child", default=None, metavar="MODE:NOISE",
                help="(child) lockstep or reuse, then off or ALPHA,EPS: time steps on request")
ap.add_argument("--sym", action="store_true", help="measure the leaf symmetry (see above)")
ap.add_argument("--sym-child", default=None, metavar="MODE:on|off",
                help="(child) one engine of --sym: lockstep or reuse, with or without leaf_symmetry")
ap.add_argument("--sym-positions", type=int, default=64, help="--sym: positions of the orientation measurement")
ap.add_argument("--forced", type=float, default=None, metavar="K", help="measure forced playouts (see above)")
ap.add_argument("--forced-noise", default="0.3,0.25", metavar="ALPHA,EPS", help="--forced: the root noise of every engine")
ap.add_argument("--forced-positions", type=int, default=512, help="--forced: positions of the share measurement")
ap.add_argument("--forced-child", default=None, metavar="MODE:off|K",
                help="(child) one engine of --forced: lockstep or reuse, the flag clear or forced_playouts=K")
ap.add_argument("--gumbel", type=int, default=None, metavar="M", help="measure the Gumbel root with sequential halving (see above)")
ap.add_argument("--gumbel-sims", default="16,32,200", help="--gumbel: the budgets of the moves/s table (comma-separated)")
ap.add_argument("--gumbel-kl-slots", type=int, default=256, help="--gumbel: games of the KL(pi' || prior) measurement (0: skip)")
ap.add_argument("--gumbel-kl-sims", type=int, default=32, help="--gumbel: simulations of the KL measurement")
ap.add_argument("--gumbel-child", default=None, metavar="MODE:off|M",
                help="(child) one engine of --gumbel: lockstep, the flag clear or gumbel_considered=M")
ap.add_argument("--leaves", default=None, metavar="K,K,...",
                help="measure leaf batching (SelfPlayEngine(leaves_per_round=K)) over --sweep-slots (see above)")
ap.add_argument("--sweep-slots", default="1,8,64,256", help="--leaves: the slot counts (comma-separated)")
ap.add_argument("--leaves-child", default=None, metavar="K,K,...",
                help="(child) one engine per K at --slots: time steps on request")
ap.add_argument("--compact", action="store_true", help="measure slot compaction over --compact-games (see above)")
ap.add_argument("--compact-games", default="512,4096", help="--compact: games = slots per iteration (comma-separated)")
ap.add_argument("--compact-noise", default="0.3,0.25", metavar="ALPHA,EPS", help="--compact: the root noise of the noisy runs")
ap.add_argument("--compact-child", default=None, metavar="on|off:NOISE",
                help="(child) compaction on or off, then off or ALPHA,EPS: one iteration of --slots games on request")
ap.add_argument("--cap", default=None, metavar="F,P", help="measure playout cap randomization (see above)")
ap.add_argument("--cap-games", type=int, default=512, help="--cap: games (= slots) of the self-play iteration")
ap.add_argument("--out", default=None)
a = ap.parse_args()
precisions = [a.precision] if a.precision else a.precisions.split(",")


def other_build(prec, library):
    """The precision a child runs that loads `library`: another build has no "f16"."""
    return "f16x3" if library and prec == "f16" else prec


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


def bind_older_build():
    """(child) Bind what the loaded library has.  A build from before the capacity / active
    count entry points runs every slot anyway: its engines call the older ones."""
    import ctypes
    from gzero import _lib
    from gzero.device import ptr, stream
    from gzero.selfplay import SelfPlayEngine
    have = ctypes.CDLL(_lib.LIB_PATH)
    _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if hasattr(have, k)}
    if hasattr(have, "gz_selfplay_puct_run_active"):
        return have

    def call(name):
        def run(self, p, n):
            assert self.n_active == self.n_slots
            _lib.check(getattr(self.lib, name)(ptr(self.d_slots), self.n_slots, ctypes.byref(p),
                                               ptr(self.pv_weights.tensor), ptr(self.d_puct_ws), int(n),
                                               ptr(self.d_records), self.record_cap, ptr(self.d_visits),
                                               ptr(self.d_counters), stream()), name)
        return run
    SelfPlayEngine._puct_run = call("gz_selfplay_puct_run")
    rounds = call("gz_selfplay_puct_rounds")
    SelfPlayEngine._puct_rounds = lambda self, n_rounds: rounds(self, self.puct, n_rounds)
    return have


def forward_only():
    import numpy as np
    import torch
    import ctypes
    from gzero import _lib, boards, device, weights
    # an older build lacks the newer entry points: bind the ones it has
    have = ctypes.CDLL(_lib.LIB_PATH)
    _lib.SIGNATURES = {k: v for k, v in _lib.SIGNATURES.items() if hasattr(have, k)}
    out = {}
    cells = np.random.default_rng(0).choice(3, size=(a.slots, 225), p=[0.8, 0.1, 0.1]).astype(np.int8)
    bl, wh = boards.cells_to_words(cells)
    d_b = torch.from_numpy(boards.leaf_words(bl, wh).view(np.int32).copy()).cuda()
    d_probs = torch.empty(a.slots * 225, device="cuda")
    d_prior = torch.empty(a.slots * 225, dtype=torch.float64, device="cuda")
    for prec in precisions:
        w = device.PVWeights(weights.pack_pv_weights(weights.init_state_dict(0)), precision=prec)
        ts = []
        for it in range(3 + 20):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            device.pv_forward_dev(w, d_b, a.slots, d_probs=d_probs, d_prior=d_prior)
            e1.record()
            torch.cuda.synchronize()
            if it >= 3:
                ts.append(e0.elapsed_time(e1))
        out[prec] = {"ms": median(ts), "min_ms": min(ts), "max_ms": max(ts), "iters": len(ts)}
    print("FORWARD_JSON " + json.dumps(out))


def bench_weights(prec, scale):
    from gzero import device, weights
    sd = weights.init_state_dict(0)
    if scale != 1.0:
        sd["policy_fc.weight"] = sd["policy_fc.weight"] * scale
        sd["policy_fc.bias"] = sd["policy_fc.bias"] * scale
    return device.PVWeights(weights.pack_pv_weights(sd), precision=prec)


def lockstep_child():
    """Per line on stdin: one lock-step step timed with device events, its ms on stdout."""
    import ctypes
    import torch
    from gzero import _lib
    from gzero.selfplay import SelfPlayEngine
    have = bind_older_build()
    eng = SelfPlayEngine(n_slots=a.slots, num_simulations=a.sims, seed=1,
                         pv_weights=bench_weights(precisions[0], a.lockstep_child), search="puct",
                         temp_plies=a.temp_plies)
    eng.advance(a.burn)
    eng.step()
    torch.cuda.synchronize()
    print("READY", flush=True)
    for line in sys.stdin:
        if line.strip() != "step":
            break
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.step()
        e1.record()
        torch.cuda.synchronize()
        assert eng.counters()["moves"] == a.slots
        print(f"STEP_MS {e0.elapsed_time(e1)!r}", flush=True)


def reuse_run(prec, scale):
    """One run: the lock-step child (started first; it idles between its steps), then
    the reuse engine; windows and steps alternate."""
    env = dict(os.environ)
    if a.lockstep_library:
        env["GZ_LIBRARY"] = os.path.abspath(a.lockstep_library)
    child = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--lockstep-child", repr(scale), "--slots",
                              str(a.slots), "--sims", str(a.sims), "--burn", str(a.burn), "--precisions",
                              other_build(prec, a.lockstep_library), "--temp-plies", str(a.temp_plies)], env=env,
                             stdin=subprocess.PIPE,
                             stdout=subprocess.PIPE, text=True)
    try:
        if child.stdout.readline().strip() != "READY":
            sys.exit(f"lock-step child failed ({child.poll()})")
        import torch
        from gzero.selfplay import SelfPlayEngine
        S, n = a.sims, a.slots
        window = 2 * (S + 1)
        eng = SelfPlayEngine(n_slots=n, num_simulations=S, seed=1, pv_weights=bench_weights(prec, scale), search="puct",
                             temp_plies=a.temp_plies, tree_reuse=True, rounds_per_step=window)
        eng.advance(a.burn)
        eng.step()
        eng.step()  # warm-up: 4 x (S+1) rounds
        torch.cuda.synchronize()
        took0 = int(eng.draws()[:, 2].sum())  # rounds the moves played so far took
        wins, steps = [], []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.step()
            e1.record()
            torch.cuda.synchronize()
            c = eng.counters()
            assert c["records_dropped"] == 0
            wins.append({"ms": e0.elapsed_time(e1), "moves": int(c["moves"]), "games": int(c["games"])})
            child.stdin.write("step\n")
            child.stdin.flush()
            line = child.stdout.readline().split()
            if len(line) != 2 or line[0] != "STEP_MS":
                sys.exit(f"lock-step child failed ({child.poll()}): {line}")
            steps.append(float(line[1]))
        took = int(eng.draws()[:, 2].sum()) - took0
    finally:
        child.stdin.close()
        child.wait(timeout=120)
    round_ms = [w["ms"] / window for w in wins]
    moves = sum(w["moves"] for w in wins)
    ms = sum(w["ms"] for w in wins)
    # the moves played in the windows and the rounds each of them took (S+1 minus the visits
    # its root inherited), from the slot statistics: slots that stay in phase play a whole
    # number of moves per window, which would quantise slots x rounds / moves
    rpm = took / moves
    rate = n / (rpm * median(round_ms) / 1e3)
    lock_round = median(steps) / (S + 1)
    out = {
        "policy_fc_scale": scale, "rounds_per_window": window, "windows": wins,
        "round_ms_median": median(round_ms), "round_ms": round_ms,
        "mean_rounds_per_move": rpm, "mean_rounds_per_move_source": "rounds taken by the moves played in the "
        "windows (slot statistics) / those moves", "slot_rounds_per_window_move": n * window * len(wins) / moves,
        "moves_per_s": rate, "moves_per_s_source": "slots / (mean rounds per move x median ms per round)",
        "moves_per_s_counted_in_windows": moves / (ms / 1e3),
        "lockstep": {"precision": other_build(prec, a.lockstep_library), "step_ms": steps,
                     "step_ms_median": median(steps), "round_ms": lock_round,
                     "rounds_per_move": S + 1, "moves_per_s": n / (median(steps) / 1e3)},
        "round_ms_over_lockstep_round_ms": median(round_ms) / lock_round,
        "measured_speedup_rounds": (S + 1) / rpm,
        "measured_speedup_moves_per_s": rate / (n / (median(steps) / 1e3)),
    }
    print(f"{prec} policy x{scale:g}: round {median(round_ms):.3f} ms (lock-step {lock_round:.3f} ms, "
          f"x{out['round_ms_over_lockstep_round_ms']:.4f}), {rpm:.1f} rounds per move (lock-step {S + 1}), "
          f"{out['moves_per_s']:.0f} moves/s (lock-step {out['lockstep']['moves_per_s']:.0f})")
    del eng
    torch.cuda.empty_cache()
    return out


def cap_run(prec, scale, F, prob):
    """One weight set: windows of the uncapped and the capped engine in turn, then one
    self-play iteration each way."""
    import time
    import numpy as np
    import torch
    import training
    from gzero.boards import RECORD_DTYPE
    from gzero.device import cap_full
    from gzero.selfplay import SelfPlayEngine
    S, n = a.sims, a.slots
    window = 2 * (S + 1)
    w = bench_weights(prec, scale)
    engines = {}
    for name, kw in (("uncapped", {}), ("capped", {"fast_simulations": F, "full_prob": prob})):
        eng = SelfPlayEngine(n_slots=n, num_simulations=S, seed=1, pv_weights=w, search="puct",
                             temp_plies=a.temp_plies, tree_reuse=True, rounds_per_step=window, **kw)
        eng.advance(a.burn)
        eng.step()
        eng.step()  # warm-up: 4 x (S+1) rounds
        torch.cuda.synchronize()
        engines[name] = (eng, int(eng.draws()[:, 2].sum()), [])
    for _ in range(a.steps):
        for name, (eng, _, wins) in engines.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            eng.step()
            e1.record()
            torch.cuda.synchronize()
            c = eng.counters()
            assert c["records_dropped"] == 0
            wins.append({"ms": e0.elapsed_time(e1), "moves": int(c["moves"]), "games": int(c["games"])})
    out = {"policy_fc_scale": scale, "rounds_per_window": window}
    for name, (eng, took0, wins) in engines.items():
        took = int(eng.draws()[:, 2].sum()) - took0
        round_ms = [x["ms"] / window for x in wins]
        moves = sum(x["moves"] for x in wins)
        rpm = took / moves
        out[name] = {"windows": wins, "round_ms": round_ms, "round_ms_median": median(round_ms),
                     "round_ms_min": min(round_ms), "round_ms_max": max(round_ms), "moves": moves,
                     "mean_rounds_per_move": rpm, "moves_per_s": n / (rpm * median(round_ms) / 1e3),
                     "moves_per_s_counted_in_windows": moves / (sum(x["ms"] for x in wins) / 1e3)}
    del engines, eng
    torch.cuda.empty_cache()
    base, cap = out["uncapped"], out["capped"]
    out["round_ms_capped_over_uncapped"] = cap["round_ms_median"] / base["round_ms_median"]
    out["uncapped_round_ms_spread"] = (base["round_ms_max"] - base["round_ms_min"]) / base["round_ms_median"]
    out["rounds_per_move_arithmetic"] = prob * (S + 1) + (1.0 - prob) * (F + 1)
    out["measured_speedup_moves_per_s"] = cap["moves_per_s"] / base["moves_per_s"]
    # one self-play iteration each way (the model only names the weights: pv_weights is given)
    games = a.cap_games
    its = {}
    for name, kw in (("warm_up", {}), ("uncapped", {}), ("capped", {"fast_simulations": F, "full_prob": prob})):
        torch.cuda.synchronize()
        t0 = time.time()
        d, d_vis, n_rec, st = training.selfplay_puct_device(games, num_simulations=S, seed=1, n_slots=games,
                                                            model="bench weights", temp_plies=a.temp_plies,
                                                            tree_reuse=True, pv_weights=w, **kw)
        torch.cuda.synchronize()
        its[name] = {"seconds": time.time() - t0, "plies": n_rec, "full_ply_records": st["full_records"],
                     "steps": st["steps"]}
        if name == "capped":
            recs = np.frombuffer(d.cpu().numpy().tobytes(), RECORD_DTYPE)
            vis = d_vis.cpu().numpy().view(np.uint16)
            full = cap_full(d.reshape(-1), 1, prob).cpu().numpy()
            # the visits a root arrived with: the previous ply's count at the move played
            # (rows are sorted by (game id, ply)); a game's first root is fresh
            prev = np.concatenate([[0], vis[np.arange(n_rec - 1), recs["move"][:-1].astype(np.int64)]]).astype(np.int64)
            prev[recs["ply"] == 0] = 0
            budget = np.where(full, S, F)
            zero = prev >= budget + 1
            its[name].update({"share_full_plies": float(full.mean()), "share_zero_simulation_plies": float(zero.mean()),
                              "share_zero_simulation_among_fast_plies": float(zero[~full].mean()),
                              "mean_visit_row_sum_fast_plies": float(vis[~full].astype(np.int64).sum(axis=1).mean())})
        del d, d_vis
    del its["warm_up"]
    out["selfplay_iteration"] = dict(its, games=games, slots=games,
                                     seconds_capped_over_uncapped=its["capped"]["seconds"] / its["uncapped"]["seconds"])
    print(f"{prec} policy x{scale:g}: round {base['round_ms_median']:.3f} ms uncapped "
          f"[{base['round_ms_min']:.3f}, {base['round_ms_max']:.3f}], {cap['round_ms_median']:.3f} ms capped; "
          f"rounds per move {base['mean_rounds_per_move']:.1f} -> {cap['mean_rounds_per_move']:.1f} "
          f"(arithmetic {out['rounds_per_move_arithmetic']:.1f}); moves/s {base['moves_per_s']:.0f} -> "
          f"{cap['moves_per_s']:.0f}; {games}-game iteration {its['uncapped']['seconds']:.2f} s "
          f"({its['uncapped']['full_ply_records']} records) -> {its['capped']['seconds']:.2f} s "
          f"({its['capped']['full_ply_records']} full of {its['capped']['plies']})", flush=True)
    return out


def noise_args(spec):
    """dirichlet_alpha / noise_eps keywords of SelfPlayEngine from "off" or "ALPHA,EPS"."""
    if spec in (None, "off"):
        return {}
    alpha, eps = (float(x) for x in spec.split(","))
    return {"dirichlet_alpha": alpha, "noise_eps": eps}


def noise_child():
    mode, spec = a.noise_child.split(":")
    step_child(mode, noise_args(spec))


def sym_child():
    mode, spec = a.sym_child.split(":")
    step_child(mode, {"leaf_symmetry": True} if spec == "on" else {})


def forced_child():
    mode, spec = a.forced_child.split(":")
    kw = noise_args(a.forced_noise)
    if spec != "off":
        kw["forced_playouts"] = float(spec)
    step_child(mode, kw)


def gumbel_child():
    mode, spec = a.gumbel_child.split(":")
    step_child(mode, {} if spec == "off" else {"gumbel_considered": int(spec)})


def spread(xs):
    return {"median": median(xs), "min": min(xs), "max": max(xs), "n": len(xs)}


def gumbel_mode_run(prec):
    kinds = [("parent", "off", a.lockstep_library), ("gumbel_off", "off", None), ("gumbel_on", str(a.gumbel), None)]
    out = three_way_run(prec, "lockstep", "--gumbel-child", kinds, "Gumbel root")
    for r in out.values():
        r["round_ms"] = spread([x / r["rounds_per_step"] for x in r["step_ms"]])
    return out


def gumbel_kernels(prec):
    """The launches of a step-API search of --slots mid-game positions, device events around
    each: per round select, the forward (PuctStepper.evaluate), backup; finish once."""
    import torch
    from gzero import device
    from gzero.selfplay import SelfPlayEngine
    n, S = a.slots, a.sims
    w = bench_weights(prec, 1.0)
    eng = SelfPlayEngine(n_slots=n, num_simulations=S, seed=1, pv_weights=w, search="puct", temp_plies=a.temp_plies)
    eng.advance(a.burn)
    st, _ = eng.boards()
    del eng
    torch.cuda.empty_cache()

    def timed(f):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = f()
        e1.record()
        return r, (e0, e1)

    out = {}
    for name, m in (("flag_clear", None), ("gumbel", a.gumbel)):
        sp = device.PuctStepper(st, list(range(n)), device.puct_params(S, 1.6, a.temp_plies, 1, prec, gumbel_considered=m))
        ev = {"select": [], "forward": [], "backup": [], "finish": []}
        for rnd in range(S + 1):
            if rnd:
                ev["select"].append(timed(sp.select)[1])
            (prior, value), e = timed(lambda: sp.evaluate(w))
            ev["forward"].append(e)
            ev["backup"].append(timed(lambda: sp.backup(prior, value))[1])
        ev["finish"].append(timed(sp.finish)[1])
        torch.cuda.synchronize()
        # (round 0's backup is the root's: with the flag it holds the root preparation)
        ms = {k: [e0.elapsed_time(e1) for e0, e1 in v] for k, v in ev.items()}
        out[name] = {k: spread(v) for k, v in ms.items()}
        out[name]["root_backup_ms"] = ms["backup"][0]
        out[name]["search_ms_sum"] = sum(sum(v) for v in ms.values())
        del sp
        torch.cuda.empty_cache()
        print(f"{prec} {name}: select {out[name]['select']['median']:.4f} ms, forward {out[name]['forward']['median']:.4f}, "
              f"backup {out[name]['backup']['median']:.4f} (root's {out[name]['root_backup_ms']:.4f}), "
              f"finish {out[name]['finish']['median']:.4f}")
    return out


def gumbel_moves(prec, S, round_ms_flagged):
    """Moves/s of a lock-step Gumbel engine at S simulations, measured, and the arithmetic
    slots / ((S + 1) x the flagged round at --sims)."""
    import torch
    from gzero.selfplay import SelfPlayEngine
    eng = SelfPlayEngine(n_slots=a.slots, num_simulations=S, seed=1, pv_weights=bench_weights(prec, 1.0), search="puct",
                         temp_plies=a.temp_plies, gumbel_considered=a.gumbel, plies_per_step=1)
    eng.advance(a.burn)
    eng.step()
    ms = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.step()
        e1.record()
        torch.cuda.synchronize()
        assert eng.counters()["moves"] == a.slots
        ms.append(e0.elapsed_time(e1))
    del eng
    torch.cuda.empty_cache()
    out = {"simulations": S, "considered": a.gumbel, "ply_ms": spread(ms), "round_ms_median": median(ms) / (S + 1),
           "moves_per_s_measured": a.slots / (median(ms) / 1e3),
           "moves_per_s_arithmetic": a.slots / ((S + 1) * round_ms_flagged / 1e3)}
    print(f"{prec} S={S} m={a.gumbel}: {out['moves_per_s_measured']:.0f} moves/s measured, "
          f"{out['moves_per_s_arithmetic']:.0f} by (S+1) x the flagged round at S={a.sims}")
    return out


def gumbel_kl(prec, scale):
    """Mean KL(pi' || prior) over the rows a lock-step Gumbel engine records: --gumbel-kl-slots
    games from the empty board played to the end, pi' = row / sum, prior = the forward's
    masked row of the record's position.  Descriptive."""
    import numpy as np
    from gzero import boards, device
    from gzero.selfplay import SelfPlayEngine
    n, S = a.gumbel_kl_slots, a.gumbel_kl_sims
    w = bench_weights(prec, scale)
    eng = SelfPlayEngine(n_slots=n, num_simulations=S, seed=1, pv_weights=w, search="puct", temp_plies=a.temp_plies,
                         gumbel_considered=a.gumbel, game_id_end=n, plies_per_step=10)
    recs, rows = [], []
    for _ in range(21):
        eng.step()
        if eng.counters()["records"]:
            recs.append(eng.records().copy())
            rows.append(eng.visits().copy())
        if sum(len(r) for r in recs) and len(set(np.concatenate(recs)["game_id"].tolist())) == n:
            break
    recs, rows = np.concatenate(recs), np.concatenate(rows).astype(np.float64)
    kl = []
    for lo in range(0, len(recs), 4096):
        r = recs[lo:lo + 4096]
        _, _, _, prior = device.pv_forward(w, boards.leaf_words(r["black"], r["white"]), want_prior=True)
        pi = rows[lo:lo + 4096] / rows[lo:lo + 4096].sum(axis=1, keepdims=True)
        on = pi > 0
        kl.append(np.where(on, pi * (np.log(np.where(on, pi, 1.0)) - np.log(np.where(on, prior, 1.0))), 0.0).sum(axis=1))
    kl = np.concatenate(kl)
    out = {"games": int(len(set(recs["game_id"].tolist()))), "rows": int(len(recs)), "simulations": S,
           "considered": a.gumbel, "kl_mean": float(kl.mean()), "kl_median": float(np.median(kl)),
           "kl_max": float(kl.max())}
    print(f"{prec} policy x{scale:g}: mean KL(pi' || prior) {out['kl_mean']:.5f} over {out['rows']} rows of {out['games']} games")
    return out


def step_child(mode, engine_kw):
    """Per line on stdin: one lock-step step (or one window of 2 x (S+1) rounds of a
    tree-reuse engine) timed with device events; its ms and moves on stdout."""
    import torch
    from gzero.selfplay import SelfPlayEngine
    bind_older_build()
    reuse = mode == "reuse"
    eng = SelfPlayEngine(n_slots=a.slots, num_simulations=a.sims, seed=1, pv_weights=bench_weights(precisions[0], 1.0),
                         search="puct", temp_plies=a.temp_plies, tree_reuse=reuse,
                         rounds_per_step=2 * (a.sims + 1) if reuse else None, **engine_kw)
    eng.advance(a.burn)
    for _ in range(2 if reuse else 1):  # warm-up (with reuse 4 x (S+1) rounds: the clocks drift apart)
        eng.step()
    torch.cuda.synchronize()
    print("READY", flush=True)
    for line in sys.stdin:
        if line.strip() != "step":
            break
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.step()
        e1.record()
        torch.cuda.synchronize()
        c = eng.counters()
        assert c["records_dropped"] == 0
        print(f"STEP_MS {e0.elapsed_time(e1)!r} {int(c['moves'])}", flush=True)


def noise_mode_run(prec, mode):
    kinds = [("parent", "off", a.lockstep_library), ("noise_off", "off", None), ("noise_on", a.noise, None)]
    return three_way_run(prec, mode, "--noise-child", kinds, "noise")


def sym_mode_run(prec, mode):
    kinds = [("parent", "off", a.lockstep_library), ("sym_off", "off", None), ("sym_on", "on", None)]
    return three_way_run(prec, mode, "--sym-child", kinds, "sym")


def forced_mode_run(prec, mode):
    kinds = [("parent", "off", a.lockstep_library), ("forced_off", "off", None), ("forced_on", repr(a.forced), None)]
    return three_way_run(prec, mode, "--forced-child", kinds, "forcing", ("--forced-noise", a.forced_noise))


def forced_shares(prec, scale):
    """What forcing and pruning do to a full search's visit row: --forced-positions mid-game
    positions (one per slot of a lock-step engine after --burn plies), each searched by
    gz_puct_search with the root noise, once with the flag clear and once set (same seed, so
    the same noise).  Raw counts come from the exported trees, the rows handed out from
    d_visits, the clean prior from a forward of the root boards.  scale: the policy FC's weight
    and bias times this (1.0: the init weights, whose prior is nearly flat; more: a synthetic
    net with a favourite move, as --reuse and --cap use)."""
    import math
    import numpy as np
    from gzero import device
    from gzero.selfplay import SelfPlayEngine
    n, S, k = a.forced_positions, a.sims, a.forced
    alpha, eps = (float(x) for x in a.forced_noise.split(","))
    w = bench_weights(prec, scale)
    eng = SelfPlayEngine(n_slots=n, num_simulations=S, seed=1, pv_weights=w, search="puct", temp_plies=a.temp_plies)
    eng.advance(a.burn)
    st, _ = eng.boards()
    del eng
    gids = list(range(n))
    live = np.flatnonzero(st["over"] == 0)
    got = {}
    for name, kk in (("flag_clear", None), ("flag_set", k)):
        p = device.puct_params(S, 1.6, 0, 1, prec, dirichlet_alpha=alpha, noise_eps=eps, forced_playouts=kk)
        _, rows, _, trees = device.puct_search(st, gids, p, w, want_trees=True)
        raw = np.zeros((n, 225), np.int64)
        noised = np.zeros((n, 225))
        for g in live:
            t = trees[g]
            kids = np.flatnonzero(np.asarray(t["parent"]) == 0)
            raw[g, np.asarray(t["move_of"])[kids]] = np.asarray(t["visits"])[kids]
            noised[g] = t["prior"][0]
        got[name] = (rows.astype(np.int64), raw, noised)
    _, _, _, clean = device.pv_forward(w, np.stack([trees[g]["board"][0] for g in range(n)]), want_prior=True)
    rows0, raw0, noised = got["flag_clear"]
    rows1, raw1, noised1 = got["flag_set"]
    assert np.array_equal(rows0, raw0) and np.array_equal(noised[live], noised1[live])
    boosted = (noised > 2.0 * clean) & (clean > 0)
    owed = np.zeros(n)
    for g in live:
        T = int(raw1[g].sum())
        for c in np.flatnonzero(raw1[g]):
            owed[g] += min(int(raw1[g, c]), math.ceil(math.sqrt((k * noised[g, c]) * T)))

    def mass(rows):
        tot = rows.sum(axis=1)
        return float(((rows * boosted).sum(axis=1)[live] / tot[live]).mean())

    out = {"positions": int(len(live)), "simulations": S, "forced_k": k, "noise": {"alpha": alpha, "eps": eps},
           "what": "shares of the S visits of a full search, means over the positions: owed = sum over root "
                   "children of min(n, ceil(forced(c))), the visits the forcing threshold covers (an upper bound "
                   "of the forced selections); displaced = sum of max(0, raw visits with the flag - raw visits "
                   "without) / S; pruned = 1 - sum(row handed out) / S; noise mass = the normalised row's mass "
                   "on cells whose noised prior exceeds twice the clean prior",
           "owed_share": float((owed[live] / S).mean()),
           "displaced_share": float((np.maximum(raw1 - raw0, 0).sum(axis=1)[live] / S).mean()),
           "pruned_share": float((1.0 - rows1.sum(axis=1)[live] / S).mean()),
           "boosted_cells_mean": float(boosted.sum(axis=1)[live].mean()),
           "noise_mass_flag_clear": mass(rows0), "noise_mass_flag_set_raw": mass(raw1),
           "noise_mass_flag_set": mass(rows1)}
    print(f"{prec} policy x{scale:g}: of {S} visits owed {out['owed_share']:.4f}, displaced {out['displaced_share']:.4f}, pruned "
          f"{out['pruned_share']:.4f}; mass on noised cells {out['noise_mass_flag_clear']:.4f} flag clear, "
          f"{out['noise_mass_flag_set_raw']:.4f} set (raw), {out['noise_mass_flag_set']:.4f} set (pruned)")
    return out


def three_way_run(prec, mode, child_flag, kinds, what, extra=()):
    """The three engines of one mode, taking turns: {name: per-step ms, moves, medians}."""
    S = a.sims
    rounds = 2 * (S + 1) if mode == "reuse" else S + 1
    off_name, on_name = kinds[1][0], kinds[2][0]
    kids = {}
    try:
        for name, spec, library in kinds:
            env = dict(os.environ)
            if library:
                env["GZ_LIBRARY"] = os.path.abspath(library)
            kids[name] = subprocess.Popen(
                [sys.executable, os.path.abspath(__file__), child_flag, f"{mode}:{spec}", "--slots", str(a.slots),
                 "--sims", str(S), "--burn", str(a.burn), "--precisions", prec, "--temp-plies", str(a.temp_plies), *extra],
                env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        for name, kid in kids.items():
            if kid.stdout.readline().strip() != "READY":
                sys.exit(f"{mode} child {name} failed ({kid.poll()})")
        out = {name: {"step_ms": [], "moves": []} for name in kids}
        for _ in range(a.steps):
            for name, kid in kids.items():
                kid.stdin.write("step\n")
                kid.stdin.flush()
                line = kid.stdout.readline().split()
                if len(line) != 3 or line[0] != "STEP_MS":
                    sys.exit(f"{mode} child {name} failed ({kid.poll()}): {line}")
                out[name]["step_ms"].append(float(line[1]))
                out[name]["moves"].append(int(line[2]))
    finally:
        for kid in kids.values():
            kid.stdin.close()
        for kid in kids.values():
            kid.wait(timeout=120)
    for name, r in out.items():
        r["step_ms_median"] = median(r["step_ms"])
        r["rounds_per_step"] = rounds
        r["round_ms_median"] = r["step_ms_median"] / rounds
    base = out["parent"]["round_ms_median"]
    for name in (off_name, on_name):
        out[name]["round_ms_over_parent"] = out[name]["round_ms_median"] / base
    print(f"{prec} {mode}: round ms parent {base:.4f}, {what} off {out[off_name]['round_ms_median']:.4f} "
          f"(x{out[off_name]['round_ms_over_parent']:.4f}), {what} on {out[on_name]['round_ms_median']:.4f} "
          f"(x{out[on_name]['round_ms_over_parent']:.4f})")
    return out


def orientation_dependence(prec):
    """Does the search depend on the board's orientation?  --sym-positions mid-game positions
    (one per slot of a lock-step engine after --burn plies), each searched as it is and
    rotated by 90 degrees (np.rot90 of the cells); the L1 distance between the visit
    distribution of the position and the rotated image's distribution rotated back, with
    the flag off and on (--sims simulations, temp_plies 0, init weights)."""
    import numpy as np
    from gzero import boards, device
    from gzero.selfplay import SelfPlayEngine
    n = a.sym_positions
    w = bench_weights(prec, 1.0)
    eng = SelfPlayEngine(n_slots=n, num_simulations=a.sims, seed=1, pv_weights=w, search="puct",
                         temp_plies=a.temp_plies)
    eng.advance(a.burn)
    st, _ = eng.boards()
    cells = boards.words_to_cells(st["black"], st["white"])
    turned = np.stack([np.rot90(c.reshape(15, 15)).reshape(225) for c in cells])
    st_t = boards.make_states(turned, n_moves=st["n_moves"], player=st["player"], over=st["over"],
                              winner=st["winner"])
    gids = list(range(n))
    live = st["over"] == 0
    out = {"positions": int(live.sum()), "plies": [int(x) for x in st["n_moves"][live]]}
    for name, flag in (("sym_off", False), ("sym_on", True)):
        p = device.puct_params(a.sims, 1.6, 0, 1, prec, leaf_symmetry=flag)
        vis = device.puct_search(st, gids, p, w)[1].astype(np.float64)[live]
        vis_t = device.puct_search(st_t, gids, p, w)[1].astype(np.float64)[live]
        back = np.stack([np.rot90(v.reshape(15, 15), k=-1).reshape(225) for v in vis_t])
        l1 = np.abs(vis / vis.sum(axis=1, keepdims=True) - back / back.sum(axis=1, keepdims=True)).sum(axis=1)
        out[name] = {"l1_mean": float(l1.mean()), "l1_median": float(np.median(l1)), "l1_max": float(l1.max()),
                     "same_move": int((vis.argmax(axis=1) == back.argmax(axis=1)).sum())}
    print(f"{prec}: L1(visits, rotated-back visits of the rotated board) over {out['positions']} positions: "
          f"{out['sym_off']['l1_mean']:.4f} without the flag, {out['sym_on']['l1_mean']:.4f} with")
    return out


def distinct_positions(prec, spec):
    """Distinct positions among the slots after --distinct-plies lock-step plies from the
    empty board at temp_plies 0."""
    import numpy as np
    import torch
    from gzero.selfplay import SelfPlayEngine
    eng = SelfPlayEngine(n_slots=a.slots, num_simulations=a.sims, seed=1, pv_weights=bench_weights(prec, 1.0),
                         search="puct", temp_plies=0, **noise_args(spec))
    for _ in range(a.distinct_plies):
        eng.step()
    st, _ = eng.boards()
    # (no game ends before its ninth ply; with more plies a slot may already be in its next game)
    first = st["n_moves"] == a.distinct_plies
    rows = np.concatenate([st["black"], st["white"]], axis=1)[first]
    n = len(np.unique(rows, axis=0))
    del eng
    torch.cuda.empty_cache()
    return {"distinct": n, "slots_in_their_first_game": int(first.sum())}


def count_rounds(eng, K, w):
    """What the engine's next step will run, from one untimed search of the same boards
    through the step API: (rounds, host reads, active rows, rows) -- the rounds by the block
    rule of gz_puct_search (unbatched: S + 1 rounds, no read)."""
    import torch
    from gzero import device
    S = a.sims
    states, gids = eng.boards()
    st = device.PuctStepper(states, gids, eng.puct)
    d_probs = torch.empty(st.rows * 225, device="cuda")
    d_prior = torch.empty(st.rows * 225, dtype=torch.float64, device="cuda")
    left, active = [], 0
    while not left or left[-1] > 0:
        if left:
            st.select()
        active += int(st.d_active.sum().item())
        _, d_value, _ = device.pv_forward_dev(w, st.d_leaves, st.rows, d_probs=d_probs, d_prior=d_prior)
        st.backup(d_prior, d_value)
        left.append(int(st.remaining().max()))
    if st.K == 0:
        assert len(left) == S + 1
        return S + 1, 0, active, (S + 1) * st.rows
    todo, ran, reads = 1 + -(-S // K), 0, 0
    while True:
        ran += todo
        reads += 1
        rest = left[min(ran, len(left)) - 1]
        if rest == 0:
            break
        todo = -(-rest // K)
    return ran, reads, active, ran * st.rows


def leaves_child():
    """One engine per K of --leaves-child at --slots.  Per "step K" on stdin: that engine's
    next step counted (count_rounds; not on a build without gz_puct_remaining, the parent's,
    whose K = 1 step is S + 1 rounds) and timed with device events."""
    import ctypes
    import torch
    from gzero import _lib
    from gzero.selfplay import SelfPlayEngine
    have = bind_older_build()
    can_count = hasattr(have, "gz_puct_remaining")
    S, n = a.sims, a.slots
    w = bench_weights(precisions[0], 1.0)
    engines = {}
    for K in (int(x) for x in a.leaves_child.split(",")):
        kw = {"leaves_per_round": K} if K > 1 else {}
        eng = SelfPlayEngine(n_slots=n, num_simulations=S, seed=1, pv_weights=w, search="puct",
                             temp_plies=a.temp_plies, **kw)
        eng.advance(a.burn)
        eng.step()
        engines[K] = eng
    torch.cuda.synchronize()
    print("READY " + torch.cuda.get_device_name(0), flush=True)
    for line in sys.stdin:
        word = line.split()
        if len(word) != 2 or word[0] != "step":
            break
        K = int(word[1])
        eng = engines[K]
        rounds, reads, active, rows = count_rounds(eng, K, w) if can_count else (S + 1, 0, -1, (S + 1) * n)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.step()
        e1.record()
        torch.cuda.synchronize()
        c = eng.counters()
        assert c["records_dropped"] == 0 and c["moves"] == n
        print(f"STEP_MS {e0.elapsed_time(e1)!r} {rounds} {reads} {active} {rows}", flush=True)


def compact_child():
    """Per "iter" on stdin: one selfplay_puct_device iteration of --slots games on --slots
    slots; a JSON line with its seconds, steps, moves, game lengths and the device time of
    the compaction launches (events around every SelfPlayEngine.compact call)."""
    import time
    import numpy as np
    import torch
    bind_older_build()
    import training
    from gzero import weights
    from gzero.boards import RECORD_DTYPE
    from gzero.selfplay import SelfPlayEngine
    from neural_network import GomokuModel
    mode, spec = a.compact_child.split(":")
    model = GomokuModel(device="cpu", precision=precisions[0])
    model.model.load_state_dict(weights.init_state_dict(0))
    model.device_weights()
    events = []
    launch = SelfPlayEngine.compact

    def timed_compact(self):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = launch(self)
        e1.record()
        events.append((e0, e1))
        return out
    SelfPlayEngine.compact = timed_compact
    noise = noise_args(spec)
    torch.cuda.synchronize()
    print("READY " + torch.cuda.get_device_name(0), flush=True)
    for line in sys.stdin:
        if line.strip() != "iter":
            break
        del events[:]
        t0 = time.perf_counter()
        d, _, n, st = training.selfplay_puct_device(a.slots, num_simulations=a.sims, seed=1, n_slots=a.slots,
                                                    model=model, temp_plies=a.temp_plies, compact=mode == "on",
                                                    **noise)
        torch.cuda.synchronize()
        sec = time.perf_counter() - t0
        recs = np.frombuffer(d.cpu().numpy().tobytes(), RECORD_DTYPE)
        length = np.bincount((recs["game_id"] - recs["game_id"].min()).astype(np.int64), minlength=a.slots)
        print("ITER " + json.dumps({"seconds": sec, "steps": st["steps"], "moves_played": st["moves_played"],
                                    "rows": n, "mean_game": float(length.mean()), "longest_game": int(length.max()),
                                    "compaction_launches": len(events),
                                    "compaction_ms": sum(e0.elapsed_time(e1) for e0, e1 in events)}), flush=True)


def compact_run(prec, games, spec):
    """The three engines of one (G, noise) cell, taking turns at one iteration each."""
    kinds = [("parent_refill", "off", a.lockstep_library), ("refill", "off", None), ("compact", "on", None)]
    kids = {}
    try:
        for name, mode, library in kinds:
            env = dict(os.environ)
            if library:
                env["GZ_LIBRARY"] = os.path.abspath(library)
            kids[name] = subprocess.Popen(
                [sys.executable, os.path.abspath(__file__), "--compact-child", f"{mode}:{spec}", "--slots", str(games),
                 "--sims", str(a.sims), "--precisions", prec, "--temp-plies", str(a.temp_plies)],
                env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        for name, kid in kids.items():
            ready = kid.stdout.readline().strip()
            if not ready.startswith("READY"):
                sys.exit(f"compact child {name} at {games} games failed ({kid.poll()})")
            device_name[0] = ready[len("READY "):]
        out = {name: {"turns": []} for name in kids}
        for _ in range(a.steps):
            for name, kid in kids.items():
                kid.stdin.write("iter\n")
                kid.stdin.flush()
                line = kid.stdout.readline()
                if not line.startswith("ITER "):
                    sys.exit(f"compact child {name} at {games} games failed ({kid.poll()}): {line}")
                out[name]["turns"].append(json.loads(line[len("ITER "):]))
                print(f"  {games} games, noise {spec}, {name}: {line.strip()}", flush=True)
    finally:
        for kid in kids.values():
            kid.stdin.close()
        for kid in kids.values():
            kid.wait(timeout=120)
    for r in out.values():
        r["seconds_median"] = median([t["seconds"] for t in r["turns"]])
    on, off = out["compact"], out["refill"]
    t = on["turns"][0]
    out["seconds_compact_over_refill"] = on["seconds_median"] / off["seconds_median"]
    out["seconds_compact_over_parent_refill"] = on["seconds_median"] / out["parent_refill"]["seconds_median"]
    out["seconds_refill_over_parent_refill"] = off["seconds_median"] / out["parent_refill"]["seconds_median"]
    out["mean_over_longest_game"] = t["mean_game"] / t["longest_game"]
    out["compaction_ms_share_of_iteration"] = median([x["compaction_ms"] / 1e3 / x["seconds"] for x in on["turns"]])
    print(f"{prec} {games} games, noise {spec}: {on['seconds_median']:.2f} s compacting, {off['seconds_median']:.2f} s "
          f"refilling (x{out['seconds_compact_over_refill']:.3f}; parent {out['parent_refill']['seconds_median']:.2f} s); "
          f"mean / longest game {t['mean_game']:.1f} / {t['longest_game']} = {out['mean_over_longest_game']:.3f}",
          flush=True)
    return out


device_name = [None]


def leaves_run(prec, slots, ks):
    """This build's engines (one per K) and the parent build's K = 1 engine at `slots`,
    taking turns at one timed step each."""
    S = a.sims
    kids = {}
    try:
        for name, spec, library in (("this", ",".join(str(k) for k in ks), None), ("parent", "1", a.lockstep_library)):
            env = dict(os.environ)
            if library:
                env["GZ_LIBRARY"] = os.path.abspath(library)
            kids[name] = subprocess.Popen(
                [sys.executable, os.path.abspath(__file__), "--leaves-child", spec, "--slots", str(slots), "--sims",
                 str(S), "--burn", str(a.burn), "--precisions", other_build(prec, library), "--temp-plies",
                 str(a.temp_plies)],
                env=env, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        for name, kid in kids.items():
            ready = kid.stdout.readline().strip()
            if not ready.startswith("READY"):
                sys.exit(f"leaves child {name} at {slots} slots failed ({kid.poll()})")
            device_name[0] = ready[len("READY "):]

        def step(name, K):
            kid = kids[name]
            kid.stdin.write(f"step {K}\n")
            kid.stdin.flush()
            line = kid.stdout.readline().split()
            if len(line) != 6 or line[0] != "STEP_MS":
                sys.exit(f"leaves child {name} at {slots} slots failed ({kid.poll()}): {line}")
            return [float(line[1])] + [int(x) for x in line[2:]]

        raw = {"parent": []}
        raw.update({K: [] for K in ks})
        for _ in range(a.steps):
            for K in ks:
                raw[K].append(step("this", K))
                raw["parent"].append(step("parent", 1))
    finally:
        for kid in kids.values():
            kid.stdin.close()
        for kid in kids.values():
            kid.wait(timeout=120)
    out = {}
    for key, rows in raw.items():
        ms = [r[0] for r in rows]
        r = {"step_ms": ms, "ms_per_move": median(ms), "rounds_per_move": [x[1] for x in rows],
             "rounds_per_move_median": median([x[1] for x in rows]),
             "ms_per_round": median([x[0] / x[1] for x in rows]), "host_reads_per_move": [x[2] for x in rows]}
        if rows[0][3] >= 0:
            r["empty_row_share"] = 1.0 - sum(x[3] for x in rows) / sum(x[4] for x in rows)
            r["forward_rows_per_round"] = rows[0][4] // rows[0][1]
        out["parent_k1" if key == "parent" else f"k{key}"] = r
    base = out["parent_k1"]["ms_per_move"]
    for key, r in out.items():
        r["ms_per_move_over_parent_k1"] = r["ms_per_move"] / base
    print(f"{prec} {slots} slots: parent K=1 {base:.2f} ms/move ({out['parent_k1']['ms_per_round']:.4f} ms/round); " +
          "; ".join(f"K={K} {out[f'k{K}']['ms_per_move']:.2f} ms/move, {out[f'k{K}']['rounds_per_move_median']:g} "
                    f"rounds, {out[f'k{K}']['ms_per_round']:.4f} ms/round, empty "
                    f"{out[f'k{K}'].get('empty_row_share', float('nan')):.3f}" for K in ks), flush=True)
    return out


if a.forward_only:
    forward_only()
    sys.exit(0)
if a.leaves_child is not None:
    leaves_child()
    sys.exit(0)
if a.compact_child is not None:
    compact_child()
    sys.exit(0)
if a.compact:
    prec = precisions[0]
    res = {"config": {"simulations": a.sims, "temp_plies": a.temp_plies, "precision": prec, "turns": a.steps,
                      "weights": "init_state_dict(0)", "noise": noise_args(a.compact_noise),
                      "what": "one training.selfplay_puct_device iteration of G games on G slots (plies_per_step 4, "
                              "lock-step), wall clock around the call; three child processes (the parent build and "
                              "this build with continuous refill, this build compacting) take turns",
                      "prediction": "mean / longest game: the share of the refill run's forward rows that belong "
                                    "to wanted games",
                      "parent_library": "another build (--lockstep-library)" if a.lockstep_library else "this build"},
           "results": {}}
    if a.note:
        res["config"]["note"] = a.note
    for games in (int(x) for x in a.compact_games.split(",") if x):
        for spec in ("off", a.compact_noise):
            res["results"][f"games_{games}_noise_{'off' if spec == 'off' else 'on'}"] = compact_run(prec, games, spec)
    if a.slots > 0:
        res["results"][f"compaction_off_step_slots_{a.slots}"] = leaves_run(prec, a.slots, [1])
    res["device"] = device_name[0]
    print("PUCT_COMPACT_JSON " + json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    sys.exit(0)
if a.leaves:
    prec = precisions[0]
    ks = [int(x) for x in a.leaves.split(",")]
    res = {"config": {"simulations": a.sims, "burn_in_plies": a.burn, "temp_plies": a.temp_plies, "precision": prec,
                      "parent_precision": other_build(prec, a.lockstep_library), "steps": a.steps, "leaves": ks,
                      "timing": "device events around one lock-step step (one move per slot); two child processes "
                                "(this build: one engine per K; the parent build: K = 1) take turns",
                      "rounds": "counted by an untimed search of the same boards through the step API before "
                                "each timed step, with gz_puct_search's block rule; empty_row_share = 1 - active "
                                "rows / (rounds x slots x K), round 0's K - 1 unused rows per game included",
                      "parent_library": "another build (--lockstep-library)" if a.lockstep_library else "this build",
                      "unchanged_path": f"{a.slots} slots, K = 1 (the flag clear) against the parent build"},
           "results": {}}
    if a.note:
        res["config"]["note"] = a.note
    for slots in (int(x) for x in a.sweep_slots.split(",") if x):
        res["results"][f"slots_{slots}"] = leaves_run(prec, slots, ks)
    if a.slots > 0:
        res["results"][f"unchanged_path_slots_{a.slots}"] = leaves_run(prec, a.slots, [1])
    res["device"] = device_name[0]
    print("PUCT_LEAVES_JSON " + json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    sys.exit(0)
if a.noise_child is not None:
    noise_child()
    sys.exit(0)
if a.sym_child is not None:
    sym_child()
    sys.exit(0)
if a.forced_child is not None:
    forced_child()
    sys.exit(0)
if a.gumbel_child is not None:
    gumbel_child()
    sys.exit(0)
if a.gumbel is not None:
    prec = precisions[0]
    res = {"config": {"slots": a.slots, "simulations": a.sims, "burn_in_plies": a.burn, "temp_plies": a.temp_plies,
                      "precision": prec, "considered": a.gumbel, "c_visit": 50.0, "c_scale": 0.5, "gumbel_scale": 1.0,
                      "steps": a.steps,
                      "timing": "device events around one lock-step step (S+1 rounds); three child processes (parent "
                                "build, this build with the flag clear and with gumbel_considered) take turns",
                      "parent_library": "another build (--lockstep-library)" if a.lockstep_library else "this build",
                      "claims": "cost per round, moves/s as (S+1) rounds per move, and a descriptive KL; nothing "
                                "about playing strength or learning"},
           "results": {}}
    if a.note:
        res["config"]["note"] = a.note
    res["results"]["lockstep"] = gumbel_mode_run(prec)
    flagged = res["results"]["lockstep"]["gumbel_on"]["round_ms_median"]
    parent = res["results"]["lockstep"]["parent"]["round_ms_median"]
    res["results"]["kernels"] = gumbel_kernels(prec)
    res["results"]["moves_per_s"] = {"parent_puct": {"simulations": a.sims,
                                                     "moves_per_s": a.slots / ((a.sims + 1) * parent / 1e3)}}
    for S in (int(x) for x in a.gumbel_sims.split(",") if x):
        res["results"]["moves_per_s"][f"S{S}_m{a.gumbel}"] = gumbel_moves(prec, S, flagged)
    res["results"]["kl"] = None
    if a.gumbel_kl_slots > 0:
        res["results"]["kl"] = {"init_weights": gumbel_kl(prec, 1.0)}
        for scale in (float(x) for x in a.policy_scale.split(",") if x):
            res["results"]["kl"][f"policy_fc_x{scale:g}_synthetic"] = gumbel_kl(prec, scale)
    import torch
    res["device"] = torch.cuda.get_device_name(0)
    print("PUCT_GUMBEL_JSON " + json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    sys.exit(0)
if a.forced is not None:
    prec = precisions[0]
    res = {"config": {"slots": a.slots, "simulations": a.sims, "burn_in_plies": a.burn, "temp_plies": a.temp_plies,
                      "precision": prec, "forced_k": a.forced, "noise": noise_args(a.forced_noise), "steps": a.steps,
                      "timing": "device events around one lock-step step (S+1 rounds) or one window of 2 x (S+1) "
                                "rounds with tree reuse; three child processes (parent build, this build with the "
                                "flag clear and with forced_playouts), all with the root noise, take turns",
                      "parent_library": "another build (--lockstep-library)" if a.lockstep_library else "this build",
                      "claims": "cost per round and what the rows show; nothing about playing strength or learning"},
           "results": {}}
    if a.note:
        res["config"]["note"] = a.note
    for mode in ("lockstep", "reuse") if a.reuse else ("lockstep",):
        res["results"][mode] = forced_mode_run(prec, mode)
    res["results"]["shares"] = None
    if a.forced_positions > 0:
        res["results"]["shares"] = {"init_weights": forced_shares(prec, 1.0)}
        for scale in (float(x) for x in a.policy_scale.split(",") if x):
            res["results"]["shares"][f"policy_fc_x{scale:g}_synthetic"] = forced_shares(prec, scale)
    import torch
    res["device"] = torch.cuda.get_device_name(0)
    print("PUCT_FORCED_JSON " + json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    sys.exit(0)
if a.sym:
    prec = precisions[0]
    res = {"config": {"slots": a.slots, "simulations": a.sims, "burn_in_plies": a.burn, "temp_plies": a.temp_plies,
                      "precision": prec, "steps": a.steps,
                      "timing": "device events around one lock-step step (S+1 rounds) or one window of 2 x (S+1) "
                                "rounds with tree reuse; three child processes (parent build, this build with the "
                                "flag clear and with leaf_symmetry) take turns",
                      "parent_library": "another build (--lockstep-library)" if a.lockstep_library else "this build"},
           "results": {}}
    if a.note:
        res["config"]["note"] = a.note
    for mode in ("lockstep", "reuse") if a.reuse else ("lockstep",):
        res["results"][mode] = sym_mode_run(prec, mode)
    if a.sym_positions > 0:
        res["results"]["orientation"] = orientation_dependence(prec)
    import torch
    res["device"] = torch.cuda.get_device_name(0)
    print("PUCT_SYM_JSON " + json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    sys.exit(0)
if a.noise:
    prec = precisions[0]
    res = {"config": {"slots": a.slots, "simulations": a.sims, "burn_in_plies": a.burn, "temp_plies": a.temp_plies,
                      "precision": prec, "noise": noise_args(a.noise), "steps": a.steps,
                      "timing": "device events around one lock-step step (S+1 rounds) or one window of 2 x (S+1) "
                                "rounds with tree reuse; three child processes (parent build, this build without "
                                "and with the noise) take turns",
                      "parent_library": "another build (--lockstep-library)" if a.lockstep_library else "this build",
                      "distinct_plies": a.distinct_plies},
           "results": {}}
    if a.note:
        res["config"]["note"] = a.note
    for mode in ("lockstep", "reuse") if a.reuse else ("lockstep",):
        res["results"][mode] = noise_mode_run(prec, mode)
    res["results"]["distinct_positions"] = {
        "what": f"distinct positions among {a.slots} games after {a.distinct_plies} plies from the empty board, "
                "temp_plies 0, lock-step",
        "noise_off": distinct_positions(prec, "off"), "noise_on": distinct_positions(prec, a.noise)}
    print(f"distinct positions after {a.distinct_plies} plies: "
          f"{res['results']['distinct_positions']['noise_off']['distinct']} without noise, "
          f"{res['results']['distinct_positions']['noise_on']['distinct']} with")
    import torch
    res["device"] = torch.cuda.get_device_name(0)
    print("PUCT_NOISE_JSON " + json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    sys.exit(0)
if a.lockstep_child is not None:
    lockstep_child()
    sys.exit(0)
if a.cap:
    prec = precisions[0]
    F, prob = a.cap.split(",")
    F, prob = int(F), float(prob)
    res = {"config": {"slots": a.slots, "simulations": a.sims, "burn_in_plies": a.burn, "temp_plies": a.temp_plies,
                      "precision": prec, "fast_simulations": F, "full_prob": prob, "steps": a.steps,
                      "warm_up_rounds": 4 * (a.sims + 1),
                      "timing": "device events around windows of 2 x (S+1) rounds; the uncapped engine (the flag "
                                "clear: the path of before) and the capped one, both of this build and in one "
                                "process, take turns; the iteration is wall clock around "
                                "training.selfplay_puct_device",
                      "claims": "cost per round, rounds per move and moves/s only; the scaled-policy runs are "
                                "synthetic and nothing is claimed about playing strength or learning"},
           "results": {}}
    if a.note:
        res["config"]["note"] = a.note
    res["results"]["init_weights"] = cap_run(prec, 1.0, F, prob)
    for scale in (float(x) for x in a.policy_scale.split(",") if x):
        res["results"][f"policy_fc_x{scale:g}_synthetic"] = cap_run(prec, scale, F, prob)
    import torch
    res["device"] = torch.cuda.get_device_name(0)
    print("PUCT_CAP_JSON " + json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    sys.exit(0)
if a.reuse:
    prec = precisions[0]
    res = {"config": {"slots": a.slots, "simulations": a.sims, "burn_in_plies": a.burn, "temp_plies": a.temp_plies,
                      "precision": prec, "warm_up_rounds": 4 * (a.sims + 1),
                      "timing": "device events around windows of 2 x (S+1) rounds; lock-step steps of a child "
                                "process alternate with the windows",
                      "lockstep_library": "another build (--lockstep-library)" if a.lockstep_library else "this build",
                      "speedup": "measured (S+1) / mean rounds per move of this run; the scaled-policy run is "
                                 "synthetic, no figure for a trained network is claimed"},
           "results": {}}
    if a.note:
        res["config"]["note"] = a.note
    res["results"]["init_weights"] = reuse_run(prec, 1.0)
    for scale in (float(x) for x in a.policy_scale.split(",") if x):
        res["results"][f"policy_fc_x{scale:g}_synthetic"] = reuse_run(prec, scale)
    import torch
    res["device"] = torch.cuda.get_device_name(0)
    print("PUCT_REUSE_JSON " + json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    sys.exit(0)

# the child first, while this process has not opened the GPU
env = dict(os.environ)
if a.forward_library:
    env["GZ_LIBRARY"] = os.path.abspath(a.forward_library)


def forward_child(env, precs):
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--forward-only", "--slots", str(a.slots),
                            "--precisions", ",".join(precs)], env=env, capture_output=True, text=True, timeout=300)
    if child.returncode != 0:
        sys.exit(f"forward-only child failed ({child.returncode}):\n{child.stdout}\n{child.stderr}")
    return json.loads([ln for ln in child.stdout.splitlines() if ln.startswith("FORWARD_JSON ")][-1][len("FORWARD_JSON "):])


# (another build has no f16: it times its f16x3 instead, and this build times the f16)
fwd = forward_child(env, list(dict.fromkeys(other_build(p, a.forward_library) for p in precisions)))
fwd_other_f16x3 = None
if a.forward_library and "f16" in precisions:
    fwd_other_f16x3 = fwd["f16x3"]
    mine = forward_child(dict(os.environ), ["f16"] + (["f16x3"] if "f16x3" not in precisions else []))
    fwd["f16"] = mine["f16"]
    if "f16x3" not in precisions:
        fwd["f16x3_this_build"] = mine["f16x3"]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from gzero import device, weights  # noqa: E402
from gzero.selfplay import SelfPlayEngine  # noqa: E402

S, n = a.sims, a.slots
res = {"config": {"slots": n, "simulations": S, "burn_in_plies": a.burn, "steps": a.steps, "temp_plies": a.temp_plies,
                  "timing": "device events; per-round times from one search driven through the step API",
                  "forward_library": "another build (--forward-library)" if a.forward_library else "this build"},
       "device": torch.cuda.get_device_name(0), "results": {}}
if a.note:
    res["config"]["note"] = a.note
for prec in precisions:
    w = device.PVWeights(weights.pack_pv_weights(weights.init_state_dict(0)), precision=prec)
    eng = SelfPlayEngine(n_slots=n, num_simulations=S, seed=1, pv_weights=w, search="puct", temp_plies=a.temp_plies)
    eng.advance(a.burn)
    eng.step()  # warm-up at the timed shape
    torch.cuda.synchronize()
    step_ms = []
    for _ in range(a.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.step()
        e1.record()
        torch.cuda.synchronize()
        step_ms.append(e0.elapsed_time(e1))
        assert eng.counters()["moves"] == n
    # per-round stage times on the same boards
    states, gids = eng.boards()
    st = device.PuctStepper(states, gids, eng.puct)
    d_probs = torch.empty(n * 225, device="cuda")
    d_prior = torch.empty(n * 225, dtype=torch.float64, device="cuda")
    ev = []
    for rnd in range(S + 1):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        if rnd:
            st.select()
        e[1].record()
        _, d_value, _ = device.pv_forward_dev(w, st.d_leaves, n, d_probs=d_probs, d_prior=d_prior)
        e[2].record()
        st.backup(d_prior, d_value)
        e[3].record()
        ev.append(e)
    torch.cuda.synchronize()
    stage = {k: [e[i].elapsed_time(e[i + 1]) for e in ev[1:]] for i, k in enumerate(("select", "forward", "backup"))}
    t = median(step_ms)
    alone = (S + 1) * fwd[prec]["ms"]
    res["results"][prec] = {
        "moves_per_s": n / (t / 1e3), "step_ms_median": t, "step_ms": step_ms, "rounds_per_step": S + 1,
        "per_round_ms": {k: {"median": median(v), "mean": float(np.mean(v)), "max": max(v)} for k, v in stage.items()},
        "stepped_search_ms": ev[0][0].elapsed_time(ev[-1][3]),
        "forward_standalone_ms": fwd[prec], "forwards_alone_ms": alone,
        "search_and_gaps_share_of_step": 1.0 - alone / t,
    }
    if prec == "f16" and fwd_other_f16x3:
        res["results"][prec]["forward_standalone_ms_f16x3_other_build"] = fwd_other_f16x3
        if "f16x3_this_build" in fwd:
            res["results"][prec]["forward_standalone_ms_f16x3_this_build"] = fwd["f16x3_this_build"]
    print(f"{prec}: {n / (t / 1e3):.0f} moves/s, step {t:.1f} ms; per round select "
          f"{median(stage['select']):.3f} / forward {median(stage['forward']):.3f} / backup "
          f"{median(stage['backup']):.3f} ms; {S + 1} standalone forwards {alone:.1f} ms")
    del eng, st
    torch.cuda.empty_cache()
print("PUCT_BENCH_JSON " + json.dumps(res))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
