"""csrc/gz_sym.h on the host, under the sanitizers.

tests/hosttest/sym_main.cpp is a stand-alone program: it is built with the host compiler
under -fsanitize=address,undefined, checks sym_src against sym_dst for all 8 x 225 cells
and on boards that touch all four edges, and prints sym_of of the known-answer rows of the
leaf-symmetry definition (include/gzero.h), which are compared here."""
import os
import shutil
import subprocess

import pytest

from conftest import REPO

ONE_STONE = [4, 3, 6, 7, 1, 3, 2, 7, 1, 1, 6, 0, 7, 6, 5, 2]  # seed 3, one black stone at cell 0..15


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_sym_header_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "sym_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(REPO, "tests", "hosttest", "sym_main.cpp"), "-o", exe], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=60)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, \
        (r.stdout[-2000:], r.stderr[-2000:])
    lines = [x for x in r.stdout.split("\n") if x.strip()]
    assert lines[0] == "ok"
    got = {(int(s), what): int(t) for _, s, what, t in (x.split() for x in lines[1:])}
    assert got[(3, "empty")] == 3 and got[(0, "empty")] == 3
    assert [got[(3, f"black{c}")] for c in range(16)] == ONE_STONE
    assert len(got) == 18
