"""pv_dg_kernel's row-class order (csrc/gz_dgclass.h dg_class_rank), on the host.

tests/hosttest/dg_class_main.cpp is built with the host compiler under
-fsanitize=address,undefined and prints the rank of the 36 (ty, tx) tap-set pairs.  The
order must be a permutation of 0..35, and on the simulation of the kernel's row sort
(tools/tile_rows_sim.py, its seeded sample of 2,400 children) it must execute at most
0.95 x the tile-taps of the round-6 order (set_rank(ty) * 6 + set_rank(tx) over
{-1,0,1}, {-1,0}, {-1}, {0,1}, {0}, {1}); the nested snake order gives 0.933."""
import importlib.util
import os
import shutil
import subprocess

import pytest

from conftest import REPO


def _sim():
    spec = importlib.util.spec_from_file_location("tile_rows_sim", os.path.join(REPO, "tools", "tile_rows_sim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_class_order_is_a_permutation_and_saves_tile_taps(tmp_path):
    exe = str(tmp_path / "dg_class")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(REPO, "tests", "hosttest", "dg_class_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-2000:]
    order = {}
    for line in r.stdout.split("\n"):
        if line.strip():
            ty, tx, k = (int(x) for x in line.split())
            order[(ty, tx)] = k
    sim = _sim()
    assert set(order) == {(a, b) for a in sim.SETS for b in sim.SETS}
    assert sorted(order.values()) == list(range(36))
    # the tool's shipped order is the kernel's
    assert all(sim.ORDERS[sim.SHIPPED](ty, tx) == k for (ty, tx), k in order.items())
    new = sim.tile_taps_per_child(lambda ty, tx: order[(ty, tx)])
    old = sim.tile_taps_per_child(sim.ORDERS["r06"])
    print(f"executed tile-taps per child: {old:.1f} (round-6 order) -> {new:.1f} ({new / old:.3f} x)")
    assert new <= 0.95 * old, (new, old)
