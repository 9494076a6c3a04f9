"""The argument checks of the C ABI are host-only: csrc/xpbd_checks.cpp and csrc/xpbd_error.cpp build with plain g++ (no hipcc,
no ROCm include path) into a stand-alone program, tests/checks_standalone_main.cpp, which makes one accepted and one refused
call of every check_* function, asserts the code returned and that the refusal's message names the `who` it was given, and
exits 0.  No GPU and no Python extension involved.

With XPBD_HOST_SANITIZE=1 the same program is also built and run under ASan + UBSan; it must leave stderr empty.  Opt-in
because a sanitizer-linked executable refuses to start where something else is preloaded into every process."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "constraint_solver_amd", "csrc")
SOURCES = [os.path.join(CSRC, "xpbd_checks.cpp"), os.path.join(CSRC, "xpbd_error.cpp"), os.path.join(ROOT, "tests", "checks_standalone_main.cpp")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
VARIANTS = {
    "plain": ["-O1"],
    "asan_ubsan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_checks_build_and_run_without_a_device(variant, tmp_path):
    sanitized = variant != "plain"
    if sanitized and os.environ.get("XPBD_HOST_SANITIZE") != "1":
        pytest.skip("set XPBD_HOST_SANITIZE=1 to build and run the checks under host sanitizers")
    exe = str(tmp_path / ("checks_standalone_" + variant))
    build = subprocess.run(["g++"] + FLAGS + VARIANTS[variant] + SOURCES + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "28 calls ok" in run.stdout
    if sanitized:
        assert run.stderr == ""


def test_the_program_calls_every_check_twice():
    declared = set(re.findall(r"\bint (check_\w+)\(", open(os.path.join(CSRC, "xpbd_checks.hpp")).read()))
    main = open(os.path.join(ROOT, "tests", "checks_standalone_main.cpp")).read()
    assert len(declared) == 14
    for name in declared:
        assert len(re.findall(r"\b(?:accepted|refused)\(%s\(" % name, main)) == 2, name


def test_the_unit_includes_no_hip_header():
    for name in ("xpbd_checks.cpp", "xpbd_checks.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and "xpbd_internal.h" not in text, name
