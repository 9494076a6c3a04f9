"""The merges of the multi-GPU world's scene queries and contact reports are host-only: csrc/xpbd_merge.hpp builds with plain
g++ (no hipcc, no ROCm include path) into a stand-alone program, tests/merge_standalone_main.cpp, which checks the ray merge
(ties in distance broken by body, a rank without hits, one rank), the overlap merge (a query one rank answers, a query three
ranks answer, empty queries, every cap from 0 -- with NULL hits -- to past the total) and the report merge (2 to 4 ranks, one
without pairs, 0 to 8 points a pair; the events against a random, an empty previous frame and from an empty frame) against
concatenate-and-sort and set differences and exits 0.  No GPU and no Python extension involved.

With XPBD_HOST_SANITIZE=1 the same program is also built and run under ASan + UBSan; it must leave stderr empty.  Opt-in
because a sanitizer-linked executable refuses to start where something else is preloaded into every process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "merge_standalone_main.cpp")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
VARIANTS = {
    "plain": ["-O1"],
    "asan_ubsan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_merges_build_and_run_without_a_device(variant, tmp_path):
    sanitized = variant != "plain"
    if sanitized and os.environ.get("XPBD_HOST_SANITIZE") != "1":
        pytest.skip("set XPBD_HOST_SANITIZE=1 to build and run the merges under host sanitizers")
    exe = str(tmp_path / ("merge_standalone_" + variant))
    build = subprocess.run(["g++"] + FLAGS + VARIANTS[variant] + SOURCES + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    if sanitized:
        assert run.stderr == ""
