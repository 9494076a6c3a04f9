"""The shard planner is host-only: csrc/xpbd_plan.cpp and csrc/xpbd_error.cpp build with plain g++ (no hipcc, no ROCm include
path) into a stand-alone program, tests/plan_standalone_main.cpp, which checks the planner's properties on a 997-body cloud
and on a 70 001-body slab (the threaded passes) and exits 0.  On the cloud it also re-plans after a motion of less than a cell
for 2, 3 and 5 ranks: the full and the light plan of every rank agree field by field, the layout of every shard (layout_shard:
local slots, source map, ghost rows, boundary slots, skip flags, joints) and the re-indexed joint records equal a brute-force
reading of the plans, and plans that do not fit together are refused.  No GPU and no Python extension involved.

With XPBD_HOST_SANITIZE=1 the same program is also built and run under ASan + UBSan and under TSan (the planner is the only
multi-threaded host code of the library); they must leave stderr empty.  Opt-in because a sanitizer-linked executable
refuses to start where something else is preloaded into every process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "constraint_solver_amd", "csrc")
SOURCES = [os.path.join(CSRC, "xpbd_plan.cpp"), os.path.join(CSRC, "xpbd_error.cpp"), os.path.join(ROOT, "tests", "plan_standalone_main.cpp")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-pthread"]
VARIANTS = {
    "plain": ["-O1"],
    "asan_ubsan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
    "tsan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=thread"],
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_planner_builds_and_runs_without_a_device(variant, tmp_path):
    sanitized = variant != "plain"
    if sanitized and os.environ.get("XPBD_HOST_SANITIZE") != "1":
        pytest.skip("set XPBD_HOST_SANITIZE=1 to build and run the planner under host sanitizers")
    exe = str(tmp_path / ("plan_standalone_" + variant))
    build = subprocess.run(["g++"] + FLAGS + VARIANTS[variant] + SOURCES + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    env = dict(os.environ, XPBD_PLAN_THREADS="4")
    run = subprocess.run([exe], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    if sanitized:
        assert run.stderr == ""
