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
ap.add_argument("--temp-plies", type=int, default=12)
ap.add_argument("--forward-library", default=None, help="libgzero.so the standalone forward is timed on")
ap.add_argument("--forward-only", action="store_true", help="(child) time gz_pv_forward alone, print JSON")
ap.add_argument("--note", default=None, help="free text stored in the result's config (e.g. which build --forward-library is)")
ap.add_argument("--out", default=None)
a = ap.parse_args()
precisions = a.precisions.split(",")


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])


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


if a.forward_only:
    forward_only()
    sys.exit(0)

# the child first, while this process has not opened the GPU
env = dict(os.environ)
if a.forward_library:
    env["GZ_LIBRARY"] = os.path.abspath(a.forward_library)
child = subprocess.run([sys.executable, os.path.abspath(__file__), "--forward-only", "--slots", str(a.slots),
                        "--precisions", a.precisions], env=env, capture_output=True, text=True, timeout=300)
if child.returncode != 0:
    sys.exit(f"forward-only child failed ({child.returncode}):\n{child.stdout}\n{child.stderr}")
fwd = json.loads([ln for ln in child.stdout.splitlines() if ln.startswith("FORWARD_JSON ")][-1][len("FORWARD_JSON "):])

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
