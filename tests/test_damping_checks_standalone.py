"""The argument checks of the damping calls and the re-index of the joint dampers by a population change are host-only:
csrc/xpbd_checks.cpp, csrc/xpbd_error.cpp and csrc/xpbd_population_remap.cpp build with plain g++ (no hipcc, no ROCm include
path) into a stand-alone program, tests/damping_checks_standalone_main.cpp, which makes every refused and every accepted call of
DampingTarget::rows (xpbd_world_set_damping) and ::dampers (xpbd_world_set_joint_damping), asserts the code returned and that each refusal's message names the `who` it was given and the
reason, holds remap_joint_set with the fourth vector of xpbd::JointSet to a restatement on 1000 random joint sets, and exits 0.
No GPU and no Python extension involved.

With XPBD_HOST_SANITIZE=1 the same program is also built and run under ASan + UBSan as an executable of its own; it must leave
stderr empty.  Opt-in because a sanitizer-linked executable refuses to start where something else is preloaded into every
process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "constraint_solver_amd", "csrc")
SOURCES = [os.path.join(CSRC, "xpbd_checks.cpp"), os.path.join(CSRC, "xpbd_error.cpp"), os.path.join(CSRC, "xpbd_population_remap.cpp"),
           os.path.join(ROOT, "tests", "damping_checks_standalone_main.cpp")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
VARIANTS = {
    "plain": ["-O1"],
    "asan_ubsan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_damping_checks_build_and_run_without_a_device(variant, tmp_path):
    sanitized = variant != "plain"
    if sanitized and os.environ.get("XPBD_HOST_SANITIZE") != "1":
        pytest.skip("set XPBD_HOST_SANITIZE=1 to build and run the checks under host sanitizers")
    exe = str(tmp_path / ("damping_checks_standalone_" + variant))
    build = subprocess.run(["g++"] + FLAGS + VARIANTS[variant] + SOURCES + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "56 checks ok, 1000 random re-index cases ok" in run.stdout
    if sanitized:
        assert run.stderr == ""


def test_every_refusal_of_the_header_is_made_by_the_program():
    """One `who` per reason the header lists for the three calls that the host-only checks decide."""
    main = open(os.path.join(ROOT, "tests", "damping_checks_standalone_main.cpp")).read()
    for who in ("null_rows", "count", "linear", "angular", "linear_cap", "angular_cap", "null_list", "range", "twice", "reserved", "mu_linear",
                "mu_angular"):
        assert 'refused(' in main and '"%s"' % who in main, who


def test_the_entry_points_check_before_they_bind_the_device():
    """In each of the three entry points the NULL world and the argument checks come before bind_device, the first call that
    touches HIP; set_joint_damping refuses a world that is not in XPBD_MODE_CONTACTS before it looks at the list."""
    text = open(os.path.join(CSRC, "xpbd_world.cpp")).read()
    for name, check in (("xpbd_world_set_damping", "}.rows("), ("xpbd_world_get_damping", "n != w->n"),
                        ("xpbd_world_set_joint_damping", "}.dampers(")):
        body = text[text.index("int %s(" % name):]
        body = body[:body.index("XPBD_ABI_CATCH")]
        assert 0 < body.index("NULL world") < body.index(check) < body.index("bind_device") < body.index("XPBD_HIP_TRY"), name
    body = text[text.index("int xpbd_world_set_joint_damping("):]
    assert body.index("need XPBD_MODE_CONTACTS") < body.index("}.dampers(")
