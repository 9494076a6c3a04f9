"""The argument checks of the kinematic calls and the re-index of the kinematic table by a population change are host-only:
csrc/xpbd_checks.cpp, csrc/xpbd_error.cpp and csrc/xpbd_population_remap.cpp build with plain g++ (no hipcc, no ROCm include
path) into a stand-alone program, tests/kinematic_checks_standalone_main.cpp, which makes every refused and every accepted call
of KinematicTarget::check / ::fixed_check (xpbd_world_set_kinematics) and KinematicTargets::check
(xpbd_world_set_kinematic_targets and its device variant), asserts the code returned and that each refusal's message names the
`who` it was given and the reason, holds remap_kinematics to a restatement on 1000 random tables, and exits 0.  No GPU and no
Python extension involved.

With XPBD_HOST_SANITIZE=1 the same program is also built and run under ASan + UBSan as an executable of its own; it must leave
stderr empty.  Opt-in because a sanitizer-linked executable refuses to start where something else is preloaded into every
process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "constraint_solver_amd", "csrc")
SOURCES = [os.path.join(CSRC, "xpbd_checks.cpp"), os.path.join(CSRC, "xpbd_error.cpp"), os.path.join(CSRC, "xpbd_population_remap.cpp"),
           os.path.join(ROOT, "tests", "kinematic_checks_standalone_main.cpp")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
VARIANTS = {
    "plain": ["-O1"],
    "asan_ubsan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_kinematic_checks_build_and_run_without_a_device(variant, tmp_path):
    sanitized = variant != "plain"
    if sanitized and os.environ.get("XPBD_HOST_SANITIZE") != "1":
        pytest.skip("set XPBD_HOST_SANITIZE=1 to build and run the checks under host sanitizers")
    exe = str(tmp_path / ("kinematic_checks_standalone_" + variant))
    build = subprocess.run(["g++"] + FLAGS + VARIANTS[variant] + SOURCES + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "80 checks ok, 1000 random re-index cases ok" in run.stdout
    if sanitized:
        assert run.stderr == ""


def test_every_refusal_of_the_header_is_made_by_the_program():
    """One `who` per reason the header lists for the two setters."""
    main = open(os.path.join(ROOT, "tests", "kinematic_checks_standalone_main.cpp")).read()
    for who in ("null_list", "no_bodies", "range", "repeat", "descent", "mode", "has_mass", "has_inertia", "finite", "zero_rotation",
                "t_null_rows", "t_count", "t_range", "t_repeat", "t_descent", "t_finite", "t_zero_rotation", "t_too_many", "t_alignment"):
        assert 'refused(' in main and '"%s"' % who in main, who


def test_the_entry_points_check_before_they_bind_the_device():
    """In each of the three setters the argument check comes before bind_device, the first call that touches HIP; a NULL world is
    refused before that (the only refusal the library itself can show without a device: tests/test_kinematic_abi.py)."""
    text = open(os.path.join(CSRC, "xpbd_world_kinematic.cpp")).read()
    for name, check in (("xpbd_world_set_kinematics", "target.check("), ("xpbd_world_set_kinematic_targets", "KinematicTargets{"),
                        ("xpbd_world_set_kinematic_targets_device", "KinematicTargets{")):
        body = text[text.index("int %s(" % name):]
        body = body[:body.index("XPBD_ABI_CATCH")]
        assert 0 < body.index("NULL world") < body.index(check) < body.index("bind_device") < body.index("XPBD_HIP_TRY"), name
