"""The frame workers of the multi-GPU world are host-only: csrc/xpbd_multi_workers.hpp (Barrier, LocalStatus, ShardJob,
FrameWorkers) and csrc/xpbd_error.cpp build with plain g++ (no hipcc, no ROCm include path) into a stand-alone program,
tests/multi_workers_standalone_main.cpp.  For pools of 1, 2 and 8 workers it runs 200 jobs each; a job passes the pool's barrier
twice, as a shard's frame does with the in-process transport, and writes (job number, k) into its own slot; every third job
worker 1 records a local error and still passes both barriers.  The program checks every slot after every job, that run() came
back only when all workers were through, that the first error in shard order is the one reported, and that a pool that never
ran and one destroyed right after a job go away cleanly.  No GPU and no Python extension involved.

With XPBD_HOST_SANITIZE=1 the same program is also built and run under TSan, and under ASan + UBSan; it must leave stderr
empty.  Opt-in because a sanitizer-linked executable refuses to start where something else is preloaded into every process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "constraint_solver_amd", "csrc")
SOURCES = [os.path.join(CSRC, "xpbd_error.cpp"), os.path.join(ROOT, "tests", "multi_workers_standalone_main.cpp")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread"]
VARIANTS = {
    "plain": ["-O1"],
    "tsan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=thread"],
    "asan_ubsan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_workers_build_and_run_without_a_device(variant, tmp_path):
    sanitized = variant != "plain"
    if sanitized and os.environ.get("XPBD_HOST_SANITIZE") != "1":
        pytest.skip("set XPBD_HOST_SANITIZE=1 to build and run the workers under host sanitizers")
    exe = str(tmp_path / ("multi_workers_standalone_" + variant))
    build = subprocess.run(["g++"] + FLAGS + VARIANTS[variant] + SOURCES + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "3 pools ok" in run.stdout
    if sanitized:
        assert run.stderr == ""


def test_the_header_includes_no_hip_header():
    text = open(os.path.join(CSRC, "xpbd_multi_workers.hpp")).read()
    assert "#include <hip" not in text and "xpbd_internal.h" not in text and "xpbd_multi.hpp" not in text
