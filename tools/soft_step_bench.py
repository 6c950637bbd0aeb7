"""Hard-label against soft-target training step, and the pi gather.

One process, interleaved rounds, device events: a NetStep.step at batch 128 with int64
labels, the same step with probability targets (gz_sgd_fc_loss_soft), and gz_dataset_pi for
a 128-sample gather.  Prints one JSON line (medians over the timed rounds), and writes it
to the path given as the first argument.

    python tools/soft_step_bench.py profiles/puct/soft_step.json
"""
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "alphazero-gomoku_amd"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gzero import _lib, sgd, weights  # noqa: E402

B, WARMUP, ROUNDS = 128, 10, 40


def main():
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    net = weights.PolicyValueNet().cuda()
    net.train()
    step = sgd.NetStep(net)
    x = (torch.rand((B, 3, 15, 15), device="cuda") < 0.3).float()
    y = torch.randint(0, 225, (B,), device="cuda")
    v = torch.rand((B, 1), device="cuda") * 2 - 1
    # visit rows of 200 simulations over ~30 cells, 4000 records, 35 % selected
    n = 4000
    vis = np.zeros((n, 225), np.int16)
    for r in range(n):
        cells = rng.choice(225, 30, replace=False)
        vis[r, cells] = rng.multinomial(200, np.ones(30) / 30)
    d_vis = torch.from_numpy(vis).cuda()
    m = int(0.35 * n)
    d_sel = torch.from_numpy(rng.choice(n, m, replace=False).astype(np.int32)).cuda()
    d_ids = torch.from_numpy(rng.integers(0, n + 8 * m, B)).cuda()
    pi = torch.empty((B, 225), dtype=torch.float32, device="cuda")
    L = _lib.load()
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def gather():
        _lib.check(L.gz_dataset_pi(ptr(d_vis), n, ptr(d_sel), m, ptr(d_ids), B, ptr(pi),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "gz_dataset_pi")

    gather()
    cases = {"hard_step_ms": lambda: step.step(x, y, v), "soft_step_ms": lambda: step.step(x, pi, v),
             "pi_gather_128_ms": gather}
    times = {k: [] for k in cases}
    for r in range(WARMUP + ROUNDS):
        for k, fn in cases.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            if r >= WARMUP:
                times[k].append(a.elapsed_time(b))
    out = {"batch": B, "rounds": ROUNDS, "warmup": WARMUP, "timing": "device events, interleaved, one process",
           "device": torch.cuda.get_device_name(0)}
    for k, t in times.items():
        out[k] = {"median": statistics.median(t), "min": min(t), "max": max(t)}
    line = json.dumps(out)
    print(line, flush=True)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
