"""The argument checks of the sensor calls are host-only: csrc/xpbd_checks.cpp and csrc/xpbd_error.cpp build with plain g++ (no
hipcc, no ROCm include path) into a stand-alone program, tests/sensor_checks_standalone_main.cpp, which makes every refused and
every accepted call of SensorTarget::table_check (xpbd_world_set_sensors, xpbd_world_get_sensors) and ::overlaps_check
(xpbd_world_sensor_overlaps and its device variant), asserts the code returned and that each refusal's message names the `who` it
was given and the reason, and exits 0.  No GPU and no Python extension involved.

With XPBD_HOST_SANITIZE=1 the same program is also built and run under ASan + UBSan as an executable of its own; it must leave
stderr empty.  Opt-in because a sanitizer-linked executable refuses to start where something else is preloaded into every
process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "constraint_solver_amd", "csrc")
SOURCES = [os.path.join(CSRC, "xpbd_checks.cpp"), os.path.join(CSRC, "xpbd_error.cpp"), os.path.join(ROOT, "tests", "sensor_checks_standalone_main.cpp")]
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off"]
VARIANTS = {
    "plain": ["-O1"],
    "asan_ubsan": ["-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"],
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_sensor_checks_build_and_run_without_a_device(variant, tmp_path):
    sanitized = variant != "plain"
    if sanitized and os.environ.get("XPBD_HOST_SANITIZE") != "1":
        pytest.skip("set XPBD_HOST_SANITIZE=1 to build and run the checks under host sanitizers")
    exe = str(tmp_path / ("sensor_checks_standalone_" + variant))
    build = subprocess.run(["g++"] + FLAGS + VARIANTS[variant] + SOURCES + ["-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "37 checks ok" in run.stdout
    if sanitized:
        assert run.stderr == ""


def test_every_refusal_of_the_header_is_made_by_the_program():
    """One `who` per reason the header lists for the setter, the getter and the two occupancy calls."""
    main = open(os.path.join(ROOT, "tests", "sensor_checks_standalone_main.cpp")).read()
    for who in ("null_table", "short_table", "long_table", "zero_n", "no_bodies", "byte_two", "byte_high", "get_null", "get_null_zero", "get_short",
                "null_sensors", "null_offsets", "null_hits", "null_n_out", "dev_null_offsets", "dev_null_hits", "no_sensor", "reports_off", "no_frame",
                "dev_no_frame"):
        assert 'refused(' in main and '"%s"' % who in main, who


def test_the_entry_points_check_before_they_bind_the_device():
    """In each call that takes arrays the argument check comes before bind_device, the first call that touches HIP; a NULL world is
    refused before that (the only refusal the library itself can show without a device: tests/test_sensor_abi.py).
    xpbd_world_get_sensors answers from the host copy and never binds the device."""
    text = open(os.path.join(CSRC, "xpbd_world_sensors.cpp")).read()
    for name, check in (("xpbd_world_set_sensors", "table_check("), ("xpbd_world_sensor_overlaps", "overlaps_check("),
                        ("xpbd_world_sensor_overlaps_device", "overlaps_check(")):
        body = text[text.index("int %s(" % name):]
        body = body[:body.index("XPBD_ABI_CATCH")]
        assert 0 < body.index("NULL world") < body.index(check) < body.index("bind_device"), name
    body = text[text.index("int xpbd_world_get_sensors("):]
    body = body[:body.index("XPBD_ABI_CATCH")]
    assert 0 < body.index("NULL world") < body.index("table_check(") and "bind_device" not in body and "hip" not in body


def test_the_unit_stays_host_only():
    for name in ("xpbd_checks.cpp", "xpbd_checks.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "SensorTarget" in text and "#include <hip" not in text and "xpbd_internal.h" not in text, name
