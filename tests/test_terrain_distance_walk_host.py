"""The ring walk of the terrain distance queries on the CPU: tests/terrain_distance_walk_check.cpp includes the unit
xpbd_terrain_query.hip, whose routines up to the per-query walk and the record are host code too, and runs the walk against the
brute-force minimum over every sample for about 15 000 points and unit cubes on five fields -- one cell, 4 x 3 at binary spacing,
9 x 7, 65 x 65 and one 10^6 away from the origin -- with max_distance 0, one cell and +inf, volumes far beside and far above the
field, and centres exactly on samples, borders and corners.  Every byte of the 96-byte record must agree.  The program is a
stand-alone executable built with its host code under AddressSanitizer and UBSan, and it runs under a time limit: a walk that does
not end fails here, not on a GPU."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_walk_equals_brute_force_on_the_host_and_always_ends(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the library cannot be built either")
    exe = str(tmp_path / "terrain_distance_walk_check")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "constraint_solver_amd", "csrc"),
                            os.path.join(HERE, "terrain_distance_walk_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)          # (a few seconds; a hung walk ends here)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert " 0 mismatches" in run.stdout and "runtime error" not in run.stderr
    counts = {k: int(v) for k, v in re.findall(r"(\w+) (\d+)[,)]", run.stdout)}
    total = int(run.stdout.split()[0])
    assert total >= 5000                                         # a few thousand points and boxes
    for kind in ("FACE_A", "FACE_B", "EDGES", "overlaps", "misses"):                  # every kind of answer went through both paths
        assert counts[kind] >= total // 50, counts
