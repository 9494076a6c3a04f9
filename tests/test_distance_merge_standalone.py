"""merge_first_hits<xpbd_distance_hit> (csrc/xpbd_merge.hpp) is host-only: it builds with plain g++ into a stand-alone program,
tests/distance_merge_standalone_main.cpp, which runs it on hand-made rows -- ties on distance broken by body, an overlap (0)
against a positive distance, a rank without hits, all misses, one rank -- and exits 0.  No GPU and no Python extension involved.

The same program is also built and run under ASan + UBSan and must leave stderr empty.  A sanitizer-linked executable refuses
to start where something else is preloaded into every process, so that variant is skipped there, and only there."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "distance_merge_standalone_main.cpp")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
VARIANTS = {
    "plain": ["-O1"],
    "asan_ubsan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}


def something_is_preloaded():
    preload_file = "/etc/ld.so.preload"
    return bool(os.environ.get("LD_PRELOAD", "").strip()) or (os.path.exists(preload_file) and os.path.getsize(preload_file) > 0)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_distance_merge_builds_and_runs_without_a_device(variant, tmp_path):
    sanitized = variant != "plain"
    if sanitized and something_is_preloaded():
        pytest.skip("a library is preloaded into every process here: a sanitizer-linked program would not start")
    exe = str(tmp_path / ("distance_merge_standalone_" + variant))
    build = subprocess.run(["g++"] + FLAGS + VARIANTS[variant] + SOURCES + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    if sanitized:
        assert run.stderr == ""
