"""Kinematic bodies without a device: the record layout against the header, the exported symbols, the Rust text and the C++
mirror, what the header says is out of scope, and the one refusal the library can show without a world (a NULL world).  Every
other refusal is the work of the host-only checks: tests/test_kinematic_checks_standalone.py."""
import ctypes as C
import os
import re

import numpy as np

import kinematic_model as km
from constraint_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "constraint_solver_amd", "csrc")
SETTERS = ["xpbd_world_set_kinematics", "xpbd_world_set_kinematic_targets", "xpbd_world_set_kinematic_targets_device"]
NEW_SYMBOLS = SETTERS + ["xpbd_world_kinematic_count"]
FIELDS = [("body", 0), ("mode", 4), ("linear", 8), ("angular", 32)]


def header():
    return open(os.path.join(ROOT, "include", "xpbd.h")).read()


def section():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    return text[text.index("KINEMATIC bodies (EXTENSION)"):text.index("typedef struct xpbd_kinematic")]


def test_entry_is_sixty_four_bytes_with_the_headers_fields():
    assert capi.KINEMATIC_DTYPE.itemsize == 64 and km.TABLE_DTYPE.itemsize == 64
    for name, at in FIELDS:
        assert capi.KINEMATIC_DTYPE.fields[name][1] == at and km.TABLE_DTYPE.fields[name][1] == at, name
    body = re.search(r"typedef struct xpbd_kinematic \{(.*?)\} xpbd_kinematic;", header(), re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[\d\])?[,;]", body) == [name for name, _ in FIELDS]
    for name, value in (("POSE", 0), ("VELOCITY", 1)):
        assert int(re.search(r"#define XPBD_KINEMATIC_%s\s+(\d+)u" % name, header()).group(1)) == value == getattr(capi, "KINEMATIC_" + name)
    assert (km.POSE, km.VELOCITY) == (capi.KINEMATIC_POSE, capi.KINEMATIC_VELOCITY)
    t = capi.kinematics([3, 5], [capi.KINEMATIC_POSE, capi.KINEMATIC_VELOCITY], [[1, 2, 3], [4, 5, 6]], [[1, 0, 0, 0], [7, 8, 9, 0]])
    assert t.tobytes() == km.table((3, km.POSE, [1, 2, 3], [1, 0, 0, 0]), (5, km.VELOCITY, [4, 5, 6], [7, 8, 9])).tobytes()


def test_the_header_defines_the_overwrite_and_names_what_is_out_of_scope():
    text = section()
    for words in ("velocity = (p_t - p) / ((double)r * h)", "dq = q_t * conjugate(q)", "half = atan2(m, dq.s)", "((2 / h) * tan(half / r) / m)",
                  "2 atan(h |w| / 2), not by h |w|", "before the broadphase", "History push and restore do not carry the table",
                  "gives the same bits", "1e-6 / h^2", "an all-zero POSE rotation", "wakes anybody"):
        assert words in text, words
    not_here = text[text.index("Not here:"):]
    for words in ("multi-GPU world", "body with mass kinematic", "fused schedule"):
        assert words in not_here, words
    edits = re.sub(r"\s*\n \*\s*", " ", header())
    edits = edits[edits.index("Not here: xpbd_multi_world_set_dynamics"):]
    assert "kinematic bodies," not in edits[:edits.index("----")]          # struck from the body edits' list
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Kinematic bodies" in design


def test_new_symbols_are_exported_and_listed():
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libxpbd_hip.so"))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.ABI_SYMBOLS, name


def test_rust_text_and_cpp_mirror_bind_the_calls():
    text = open(os.path.join(ROOT, "constraint_solver_amd", "ffi", "xpbd_ffi.rs")).read()
    body = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct XpbdKinematic \{(.*?)\}", text, re.S).group(1)
    assert re.findall(r"pub (\w+): ([\w\[\]; ]+),", body) == [("body", "u32"), ("mode", "u32"), ("linear", "[f64; 3]"), ("angular", "[f64; 4]")]
    for name, value in (("POSE", 0), ("VELOCITY", 1)):
        assert int(re.search(r"pub const XPBD_KINEMATIC_%s: u32 = (\d+);" % name, text).group(1)) == value
    for name in SETTERS:
        args = [a.strip() for a in re.search(r"pub fn %s\((.*?)\)\s*-> c_int;" % name, text, re.S).group(1).split(",")]
        assert args[0] == "w: *mut XpbdWorld" and "n: u32" in args, name
    assert re.search(r"pub fn xpbd_world_kinematic_count\(w: \*const XpbdWorld\) -> u32;", text)
    host = open(os.path.join(ROOT, "constraint_solver_amd", "host", "constraint_solver.hpp")).read()
    for name in SETTERS:
        assert re.search(r"check\(%s\(w_, " % name, host), name
    assert "xpbd_world_kinematic_count(w_)" in host


def test_null_world_is_rejected_without_a_device():
    L = capi.hip_lib()
    table = km.table((0, km.POSE, [0, 0, 0], [1, 0, 0, 0]))
    idx, rows = np.zeros(1, dtype=np.uint32), np.zeros(7)
    calls = {
        "xpbd_world_set_kinematics": (table.ctypes.data, 1),
        "xpbd_world_set_kinematic_targets": (idx.ctypes.data, rows.ctypes.data, 1),
        "xpbd_world_set_kinematic_targets_device": (idx.ctypes.data, rows.ctypes.data, 1),
    }
    for name, args in calls.items():
        assert getattr(L, name)(None, *args) == capi.E_INVALID, name
        message = L.xpbd_last_error()
        assert b"NULL world" in message and name.encode() in message, (name, message)
        assert getattr(L, name)(None, *args[:-1], 0) == capi.E_INVALID, name      # ... also with n == 0, which a live world accepts
    assert L.xpbd_world_kinematic_count(None) == 0


def test_the_units_are_listed_where_the_others_are():
    build = open(os.path.join(ROOT, "constraint_solver_amd", "_build.py")).read()
    assert '"xpbd_kinematic.hip"' in build and '"xpbd_world_kinematic.cpp"' in build
    hip = open(os.path.join(CSRC, "xpbd_kinematic.hip")).read()
    for kernel in ("k_kinematic_velocities", "k_kinematic_retarget"):
        assert "__global__ void __launch_bounds__(kBlock) %s(" % kernel in hip, kernel
    assert "__shared__" not in hip and "atomic" not in hip.replace("no atomics", "").replace("no\n// atomics", "")
