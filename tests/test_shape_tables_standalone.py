"""The compiler of the shape tables is host-only: csrc/xpbd_shape_tables.cpp and csrc/xpbd_error.cpp build with plain g++ (no
hipcc, no ROCm include path) into a stand-alone program, tests/shape_tables_standalone_main.cpp, which holds compile_polytopes to
a naive restatement bit for bit (a tetrahedron, a cube in both windings, two prisms, an empty shape, 300 tables of random
hulls), makes one refused call per message next to the accepted neighbour, and exits 0.  No GPU and no Python extension involved.

With XPBD_HOST_SANITIZE=1 the same program is also built and run under ASan + UBSan; it must leave stderr empty.  Opt-in
because a sanitizer-linked executable refuses to start where something else is preloaded into every process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "constraint_solver_amd", "csrc")
SOURCES = [os.path.join(CSRC, "xpbd_shape_tables.cpp"), os.path.join(CSRC, "xpbd_error.cpp"), os.path.join(ROOT, "tests", "shape_tables_standalone_main.cpp")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
VARIANTS = {
    "plain": ["-O1"],
    "asan_ubsan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_shape_tables_build_and_run_without_a_device(variant, tmp_path):
    sanitized = variant != "plain"
    if sanitized and os.environ.get("XPBD_HOST_SANITIZE") != "1":
        pytest.skip("set XPBD_HOST_SANITIZE=1 to build and run the compiler under host sanitizers")
    exe = str(tmp_path / ("shape_tables_standalone_" + variant))
    build = subprocess.run(["g++"] + FLAGS + VARIANTS[variant] + SOURCES + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "309 tables ok, 21 refusals ok" in run.stdout
    if sanitized:
        assert run.stderr == ""


def test_the_unit_includes_no_hip_header():
    for name in ("xpbd_shape_tables.cpp", "xpbd_shape_tables.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "xpbd_internal.h" not in text, name
