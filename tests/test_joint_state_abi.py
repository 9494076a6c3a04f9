"""Joint states and drive targets without a device: the record layout against the header, the exported symbols, the Rust text
and the C++ mirror, and every argument error of the four calls, all of them returned before any device work.

Without a device no world can be created, so only the NULL world can be refused through the library itself.  The other
refusals -- a NULL out or NULL targets with n > 0, a NULL list with n other than the count, an index out of range, a list that
does not ascend, a non-finite target, an ANGLE target outside [-pi, pi] -- are the work of JointStateTarget::check and
DriveTargets::check (csrc/xpbd_checks.cpp), which need no device: tests/joint_state_standalone_main.cpp builds them with plain
g++ into a program of its own and makes every refused and every accepted call.  The same program checks the drive -> item map
of build_extra_tables (csrc/xpbd_population_remap.cpp), which xpbd_world_set_drive_targets edits the resident items through."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

from constraint_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "constraint_solver_amd", "csrc")
NEW_SYMBOLS = ["xpbd_world_joint_states", "xpbd_world_joint_states_device", "xpbd_world_set_drive_targets", "xpbd_world_set_drive_targets_device"]
FIELDS = [("separation", 0), ("misalignment", 8), ("angle", 16), ("angle_rate", 24), ("travel", 32), ("travel_rate", 40), ("swing", 48),
          ("twist", 56), ("joint", 64), ("kind", 68), ("flags", 72), ("reserved", 76)]
FLAGS = ["HAS_ANGLE", "HAS_TRAVEL", "HAS_SWING", "HAS_TWIST", "ANGLE_OF_DRIVE", "ANGLE_BELOW", "ANGLE_ABOVE", "TRAVEL_BELOW", "TRAVEL_ABOVE",
         "SWING_ABOVE", "TWIST_BELOW", "TWIST_ABOVE", "NO_JOINT"]


def header():
    return open(os.path.join(ROOT, "include", "xpbd.h")).read()


def test_state_record_is_eighty_bytes_with_the_headers_fields_and_flags():
    assert capi.JOINT_STATE_DTYPE.itemsize == 80
    for name, at in FIELDS:
        assert capi.JOINT_STATE_DTYPE.fields[name][1] == at, name
    body = re.search(r"typedef struct xpbd_joint_state \{(.*?)\} xpbd_joint_state;", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)[,;]", body) == [name for name, _ in FIELDS]
    values = set()
    for flag in FLAGS:
        value = int(re.search(r"#define XPBD_JOINT_STATE_%s\s+(0x[0-9A-Fa-f]+)u" % flag, header()).group(1), 16)
        assert getattr(capi, "JOINT_STATE_" + flag) == value, flag
        values.add(value)
    assert len(values) == len(FLAGS)                                    # no two share a bit


def test_the_header_names_what_is_out_of_scope():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    section = text[text.index("Joint STATES and drive TARGETS"):text.index("typedef struct xpbd_joint_state")]
    not_here = section[section.index("Not here:"):]
    for words in ("multi-GPU world", "compliance or max_force in place", "multi-turn angle counting", "joint reactions"):
        assert words in not_here, words
    assert "History push and restore do not carry targets" in section and "[-pi, pi] never binds" in section


def test_new_symbols_are_exported_and_listed():
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libxpbd_hip.so"))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.ABI_SYMBOLS, name


def test_rust_text_and_cpp_mirror_bind_the_four_calls():
    text = open(os.path.join(ROOT, "constraint_solver_amd", "ffi", "xpbd_ffi.rs")).read()
    body = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct XpbdJointState \{(.*?)\}", text, re.S).group(1)
    fields = re.findall(r"pub (\w+): (\w+),", body)
    assert fields == [(name, "f64" if at < 64 else "u32") for name, at in FIELDS]
    for flag in FLAGS:
        value = int(re.search(r"pub const XPBD_JOINT_STATE_%s: u32 = 0x([0-9A-Fa-f_]+);" % flag, text).group(1).replace("_", ""), 16)
        assert value == getattr(capi, "JOINT_STATE_" + flag), flag
    for name in NEW_SYMBOLS:
        args = [a.strip() for a in re.search(r"pub fn %s\((.*?)\)\s*-> c_int;" % name, text, re.S).group(1).split(",")]
        assert args[0] == "w: *mut XpbdWorld" and args[1].endswith("*const u32") and "n: u32" in args, name
    host = open(os.path.join(ROOT, "constraint_solver_amd", "host", "constraint_solver.hpp")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"check\(%s\(w_, " % name, host), name


def test_null_world_is_rejected_without_a_device():
    L = capi.hip_lib()
    idx = np.arange(3, dtype=np.uint32)
    out = np.zeros(3, dtype=capi.JOINT_STATE_DTYPE)
    targets = np.zeros(3)
    calls = {
        "xpbd_world_joint_states": (idx.ctypes.data, 3, out.ctypes.data),
        "xpbd_world_joint_states_device": (idx.ctypes.data, 3, out.ctypes.data),
        "xpbd_world_set_drive_targets": (idx.ctypes.data, targets.ctypes.data, 3),
        "xpbd_world_set_drive_targets_device": (idx.ctypes.data, targets.ctypes.data, 3),
    }
    assert sorted(calls) == sorted(NEW_SYMBOLS)
    for name, args in calls.items():
        assert getattr(L, name)(None, *args) == capi.E_INVALID, name
        message = L.xpbd_last_error()
        assert b"NULL world" in message and name.encode() in message, (name, message)
        empty = tuple(0 if isinstance(a, int) and a == 3 else a for a in args)   # ... also with n == 0, which a live world accepts
        assert getattr(L, name)(None, *empty) == capi.E_INVALID, name
    assert not out.view(np.uint8).any()                                 # nothing was written


def test_every_other_refusal_and_the_drive_item_map_without_a_device(tmp_path):
    sources = [os.path.join(CSRC, "xpbd_checks.cpp"), os.path.join(CSRC, "xpbd_error.cpp"), os.path.join(CSRC, "xpbd_population_remap.cpp"),
               os.path.join(ROOT, "tests", "joint_state_standalone_main.cpp")]
    exe = str(tmp_path / "joint_state_standalone")
    build = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-ffp-contract=off", "-O1"] + sources + ["-o", exe],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "28 checks ok, 1000 random cases ok" in run.stdout


def test_the_entry_points_check_before_they_bind_the_device():
    """In each of the four definitions the argument check comes before bind_device, the first call that touches HIP."""
    text = open(os.path.join(CSRC, "xpbd_world_joint_state.cpp")).read()
    for name, check in zip(NEW_SYMBOLS, ("JointStateTarget{", "JointStateTarget{", "DriveTargets{", "DriveTargets{")):
        body = text[text.index("int %s(" % name):]
        body = body[:body.index("XPBD_ABI_CATCH")]
        assert 0 < body.index("NULL world") < body.index(check) < body.index("bind_device") < body.index("XPBD_HIP_TRY"), name
