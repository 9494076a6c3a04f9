"""The argument checks of the mass edits are host-only: csrc/xpbd_checks.cpp and csrc/xpbd_error.cpp build with plain g++ (no
hipcc, no ROCm include path) into a stand-alone program, tests/mass_edit_checks_standalone_main.cpp, which makes every refused and
every accepted call of MassEditTarget::check (xpbd_world_set_mass_properties and its device variant) and ::get_check
(xpbd_world_get_mass_properties), asserts the code returned -- XPBD_E_INVALID, or XPBD_E_SINGULAR_INERTIA for a singular DIRECT
tensor -- and that each refusal's message names the `who` it was given and the reason, runs the row rules the kernel shares
(csrc/xpbd_mass_row.hpp) on known answers, and exits 0.  No GPU and no Python extension involved.

With XPBD_HOST_SANITIZE=1 the same program is also built and run under ASan + UBSan as an executable of its own; it must leave
stderr empty.  Opt-in because a sanitizer-linked executable refuses to start where something else is preloaded into every
process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "constraint_solver_amd", "csrc")
SOURCES = [os.path.join(CSRC, "xpbd_checks.cpp"), os.path.join(CSRC, "xpbd_error.cpp"), os.path.join(ROOT, "tests", "mass_edit_checks_standalone_main.cpp")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
VARIANTS = {
    "plain": ["-O1"],
    "asan_ubsan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}
N_CHECKS = 129


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_mass_edit_checks_build_and_run_without_a_device(variant, tmp_path):
    sanitized = variant != "plain"
    if sanitized and os.environ.get("XPBD_HOST_SANITIZE") != "1":
        pytest.skip("set XPBD_HOST_SANITIZE=1 to build and run the checks under host sanitizers")
    exe = str(tmp_path / ("mass_edit_checks_standalone_" + variant))
    build = subprocess.run(["g++"] + FLAGS + VARIANTS[variant] + SOURCES + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "%d checks ok" % N_CHECKS in run.stdout
    if sanitized:
        assert run.stderr == ""


def test_every_refusal_of_the_header_is_made_by_the_program():
    """One `who` per reason the header lists for the three calls."""
    main = open(os.path.join(ROOT, "tests", "mass_edit_checks_standalone_main.cpp")).read()
    for who in ("null_rows", "no_bodies", "count", "range", "twice", "flag_bits", "layout", "finite", "negative", "zero_mass", "negative_mass",
                "singular_row", "singular_columns", "singular_zero", "kinematic_mass", "kinematic_direct", "kinematic_inertia",
                "d_null_rows", "d_no_bodies", "d_count", "d_too_many", "d_alignment", "d_flag_bits", "d_layout",
                "g_null_rows", "g_no_bodies", "g_count", "g_range"):
        assert 'refused(' in main and '"%s"' % who in main, who


def test_the_entry_points_check_before_they_bind_the_device():
    """In each of the three calls the argument check comes before bind_device, the first call that touches HIP; a NULL world is
    refused before that (the only refusal the library itself can show without a device: tests/test_mass_edit_abi.py)."""
    text = open(os.path.join(CSRC, "xpbd_world_edit.cpp")).read()
    for name, check in (("xpbd_world_set_mass_properties", ".check(who, indices, n, rows, flags, true)"),
                        ("xpbd_world_set_mass_properties_device", ".check(who, dev_indices, n, dev_rows, flags, false)"),
                        ("xpbd_world_get_mass_properties", ".get_check(who, indices, n, rows)")):
        body = text[text.index("int %s(" % name):]
        body = body[:body.index("XPBD_ABI_CATCH")]
        assert 0 < body.index("NULL world") < body.index(check) < body.index("bind_device") < body.index("XPBD_HIP_TRY"), name
    # the host variant's kinematic rule reads the host copy of the table, the kernel the device table
    assert "w->kinematics.list.data()" in text and "w->kinematics.view()" in text
    # ... and both variants drop the contact pipeline's copies of the mass properties
    edit = text[text.index("int enqueue_mass_edit("):text.index("int xpbd_world_set_mass_properties(")]
    assert "w->stat_shared = false;" in edit and "w->stat_rec_valid = false;" in edit
    assert edit.index("w->sleep.request(") < edit.index("launch_set_mass(")        # the wake requests see the old mass properties
