"""The terrain walk of the scene queries on the CPU: tests/terrain_walk_check.cpp includes the unit xpbd_terrain_query.hip, whose
routines up to terrain_cast are host code too, and runs the walk against the brute-force minimum over all triangles for about
21 000 random and crafted rays on five fields -- corners, grid lines, diagonals, origins 2^60 away, and direction components so
small (5e-324, 1e-320, 1e-306) that a border's t overflows to +inf.  The program is a stand-alone executable built with its host
code under AddressSanitizer and UBSan, and it runs under a time limit: a walk that does not end fails here, not on a GPU."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_walk_equals_brute_force_on_the_host_and_always_ends(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the library cannot be built either")
    exe = str(tmp_path / "terrain_walk_check")
    build = subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-Xarch_host", "-fsanitize=address,undefined",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "constraint_solver_amd", "csrc"),
                            os.path.join(HERE, "terrain_walk_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)          # (about a second; a hung walk ends here)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
    assert " 0 mismatches" in run.stdout and "runtime error" not in run.stderr
    tiny = int(run.stdout.split("(")[1].split()[0])
    assert tiny >= 2000
