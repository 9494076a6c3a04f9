"""merge_first_hits (csrc/xpbd_merge.hpp) is one template for the three records with a (distance, body) order -- xpbd_ray_hit,
xpbd_sweep_hit, xpbd_distance_hit.  tests/first_hits_merge_standalone_main.cpp instantiates it for all three over the same rows
-- a tie on distance decided by the body, a miss at +inf, one rank, no queries -- and the three must name the same winners, the
ones written down here.  Plain g++, no GPU and no Python extension involved.

The same program is also built and run under ASan + UBSan and must leave stderr empty.  A sanitizer-linked executable refuses
to start where something else is preloaded into every process, so that variant is skipped there, and only there."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "first_hits_merge_standalone_main.cpp")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
VARIANTS = {
    "plain": ["-O1"],
    "asan_ubsan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}
NO_HIT = 0xFFFFFFFF
WINNERS = ["1.5 4", "0 2", "0.25 6", "8 5", "inf %d" % NO_HIT]  # (distance, body) of the five queries


def something_is_preloaded():
    preload_file = "/etc/ld.so.preload"
    return bool(os.environ.get("LD_PRELOAD", "").strip()) or (os.path.exists(preload_file) and os.path.getsize(preload_file) > 0)


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_the_three_record_types_merge_to_the_same_winners(variant, tmp_path):
    sanitized = variant != "plain"
    if sanitized and something_is_preloaded():
        pytest.skip("a library is preloaded into every process here: a sanitizer-linked program would not start")
    exe = str(tmp_path / ("first_hits_merge_standalone_" + variant))
    build = subprocess.run(["g++"] + FLAGS + VARIANTS[variant] + SOURCES + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    lines = run.stdout.splitlines()
    assert lines == ["winner %d: %s" % (q, w) for q, w in enumerate(WINNERS)] + ["first_hits_merge_standalone ok"]
    if sanitized:
        assert run.stderr == ""
