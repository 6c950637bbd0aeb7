"""bench.py --dump-outputs and the plain / --full split.

* collect_outputs (what --dump-outputs writes) of two engines built from the same
  arguments: the integer-valued arrays (counters, slots, records, sampled boards and
  their kinds) are equal, the forward's outputs agree within 2 x 2e-5 (each run is
  within DELTA_TOL = 2e-5 of the full forward, tests/test_gpu_pvinc.py); the sampled
  rows are the forward of the sampled boards (full forward of the same boards, 2e-5).
* a plain `bench.py --gpus 1 --steps 2 --warmup 1 --dump-outputs DIR` at a small size:
  one JSON line with the headline's fields and none of --full's blocks, DIR/<name>.npy
  in float32 / float64 within the 64 MB limit.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO, SEED
from gzero import weights

pytestmark = pytest.mark.gpu

DELTA_TOL = 2e-5  # as tests/test_gpu_pvinc.py
SMALL = ["--slots", "64", "--sims", "50", "--burn-in", "20"]
FULL_ONLY = ("cpu_baseline", "config4", "config5", "fp32", "prior_elided")
NAMES = ("counters", "slot_state", "slot_boards", "records", "leaves", "leaf_kind", "logits", "value", "probs",
         "prior")


def _engine_outputs():
    import bench
    from gzero.device import PVWeights
    from gzero.selfplay import SelfPlayEngine
    w = PVWeights(weights.pack_pv_weights(weights.init_state_dict(0)), precision="f16x3")
    eng = SelfPlayEngine(n_slots=64, num_simulations=50, c_puct=1.6, exploration=0.05, beta=0.0, seed=SEED,
                         pv_weights=w, plies_per_step=1, pv_mode="tree")
    eng.advance(20)
    eng.step()
    eng.step()
    return bench.collect_outputs(eng, SEED, sample=512), w


def test_collect_outputs_same_arguments_same_arrays():
    from gzero import device
    a, w = _engine_outputs()
    b, _ = _engine_outputs()
    assert set(a) == set(b) == set(NAMES)
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), (name, a[name].dtype)
        assert a[name].shape == b[name].shape, name
    k = len(a["leaves"])
    assert k == 512 and a["counters"][4] == 64 and a["slot_boards"].shape == (64, 16)
    assert a["logits"].shape == (k, 225) and a["prior"].shape == (k, 225) and a["prior"].dtype == np.float64
    assert set(np.unique(a["leaf_kind"])) >= {0.0, 1.0}, "roots and root children are in the sample"
    for name in ("counters", "slot_state", "slot_boards", "records", "leaves", "leaf_kind"):
        assert np.array_equal(a[name], b[name]), name
    for name in ("logits", "value", "probs", "prior"):
        d = float(np.abs(a[name].astype(np.float64) - b[name].astype(np.float64)).max())
        print(f"{name}: max |run a - run b| = {d:.2e}")
        assert d <= 2 * DELTA_TOL, (name, d)
    # the sampled rows belong to the sampled boards
    lg, v, _ = device.pv_forward(w, a["leaves"].astype(np.uint32))
    e = (float(np.abs(lg - a["logits"]).max()), float(np.abs(v - a["value"]).max()))
    print("sample vs full forward of the sampled boards: logits %.2e value %.2e" % e)
    assert e[0] < DELTA_TOL and e[1] < DELTA_TOL, e


def test_bench_plain_run_dumps_outputs(tmp_path):
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(out)] + SMALL, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["steps"] == 2 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    # 2 steps x 64 slots x 1 ply in 2 x ms_per_step
    assert d["value"] == pytest.approx(64 * 1e3 / d["ms_per_step"], rel=1e-3)
    assert not [k for k in FULL_ONLY if k in d], "a plain run holds none of --full's blocks"
    names = sorted(p.name for p in out.iterdir())
    assert names == sorted(n + ".npy" for n in NAMES)
    total = 0
    for n in names:
        a = np.load(out / n)
        assert a.dtype in (np.float32, np.float64), (n, a.dtype)
        assert np.isfinite(a).all(), n
        total += a.nbytes
    assert 0 < total <= 64 * 1024 * 1024
    assert np.load(out / "counters.npy")[4] == 64  # the last step's plies
