"""Damping without a device: the record layouts against the header, the exported symbols, the Rust text and the C++ mirror, what
the header defines and what it says is out of scope, and the one refusal the library can show without a world (a NULL world).
Every other refusal is the work of the host-only checks: tests/test_damping_checks_standalone.py."""
import ctypes as C
import os
import re

import numpy as np

import damping_model as dm
from constraint_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "constraint_solver_amd", "csrc")
NEW_SYMBOLS = ["xpbd_world_set_damping", "xpbd_world_get_damping", "xpbd_world_set_joint_damping"]


def header():
    return open(os.path.join(ROOT, "include", "xpbd.h")).read()


def section():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    return text[text.index("DAMPING (EXTENSION)"):text.index("typedef struct xpbd_body_damping")]


def fields_of(struct):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), header(), re.S).group(1)
    return re.findall(r"(\w+)[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))


def test_the_records_have_the_headers_fields():
    assert capi.BODY_DAMPING_DTYPE.itemsize == 32 == dm.ROW_DTYPE.itemsize
    assert capi.JOINT_DAMPING_DTYPE.itemsize == 24 == dm.JOINT_DAMPING_DTYPE.itemsize
    assert list(capi.BODY_DAMPING_DTYPE.names) == fields_of("xpbd_body_damping") == list(dm.ROW_DTYPE.names)
    assert list(capi.JOINT_DAMPING_DTYPE.names) == fields_of("xpbd_joint_damping") == list(dm.JOINT_DAMPING_DTYPE.names)
    assert [capi.JOINT_DAMPING_DTYPE.fields[n][1] for n in capi.JOINT_DAMPING_DTYPE.names] == [0, 4, 8, 16]
    rows = capi.body_damping(3, linear=[0.0, 1.0, 2.0], max_angular_speed=5.0)
    assert rows.tobytes() == dm.rows(3, linear=[0.0, 1.0, 2.0], max_angular_speed=5.0).tobytes()
    assert capi.body_damping(2).tobytes() == np.array([dm.DEFAULT_ROW] * 2, dtype=dm.ROW_DTYPE).tobytes()
    assert capi.joint_damping([4, 1], 2.0, [0.0, 3.0]).tobytes() == dm.dampers((4, 2.0, 0.0), (1, 2.0, 3.0)).tobytes()


def test_the_header_defines_the_pass_and_names_what_is_out_of_scope():
    text = section()
    for words in ("stage 7 of every substep", "k = (mu * h < 1.0) ? mu * h : 1.0", "lambda = (k_l * len) / Wsum", "lambda = (k_a * len) / Wang",
                  "q_a * (inverse_inertia_a * (conjugate(q_a) * (lambda * n)))", "v = v + dv / count", "s_l = 1.0 / (1.0 + h * c_l)",
                  "if (m > max_linear_speed) v = v * (max_linear_speed / m)", "where the two ends' counts differ", "Off means off",
                  "S (h c)^2 / 2", "wake every body", "re-indexes it with the joints", "accept xpbd_world_set_damping and ignore the values"):
        assert words in text, words
    not_here = text[text.index("Not here:"):]
    for words in ("multi-GPU world", "in place or on the device", "pinned reference modes", "drives on ball joints", "joint reactions", "part of a group"):
        assert words in not_here, words
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "### Damping" in design and "k_body_damping" in design
    assert "xpbd_world_set_damping" in open(os.path.join(ROOT, "README.md")).read()


def test_new_symbols_are_exported_and_listed():
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libxpbd_hip.so"))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.ABI_SYMBOLS, name


def test_rust_text_and_cpp_mirror_bind_the_calls():
    text = open(os.path.join(ROOT, "constraint_solver_amd", "ffi", "xpbd_ffi.rs")).read()
    body = re.search(r"pub struct XpbdBodyDamping \{(.*?)\}", text, re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", body) == [(n, "f64") for n in fields_of("xpbd_body_damping")]
    body = re.search(r"pub struct XpbdJointDamping \{(.*?)\}", text, re.S).group(1)
    assert re.findall(r"pub (\w+): (\w+),", body) == [("joint", "u32"), ("reserved", "u32"), ("linear", "f64"), ("angular", "f64")]
    for name in NEW_SYMBOLS:
        args = [a.strip() for a in re.search(r"pub fn %s\((.*?)\)\s*-> c_int;" % name, text, re.S).group(1).split(",")]
        assert args[0] == "w: *mut XpbdWorld" and args[-1] == "n: u32", name
    host = open(os.path.join(ROOT, "constraint_solver_amd", "host", "constraint_solver.hpp")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"check\(%s\(w_, " % name, host), name


def test_null_world_is_rejected_without_a_device():
    L = capi.hip_lib()
    rows, list_ = capi.body_damping(1, linear=1.0), capi.joint_damping([0], 1.0, 1.0)
    for name, data in (("xpbd_world_set_damping", rows), ("xpbd_world_get_damping", rows), ("xpbd_world_set_joint_damping", list_)):
        for n in (1, 0):                                              # ... also with n == 0, which a live world accepts
            assert getattr(L, name)(None, data.ctypes.data, n) == capi.E_INVALID, name
            message = L.xpbd_last_error()
            assert b"NULL world" in message and name.encode() in message, (name, message)


def test_the_unit_is_listed_where_the_others_are_and_uses_no_lds_or_atomics():
    build = open(os.path.join(ROOT, "constraint_solver_amd", "_build.py")).read()
    assert '"xpbd_damping.hip"' in build
    hip = open(os.path.join(CSRC, "xpbd_damping.hip")).read()
    for kernel in ("k_body_damping", "k_joint_damping"):
        assert "__global__ void __launch_bounds__(kBlock) %s(" % kernel in hip, kernel
    code = re.sub(r"//.*", "", hip)
    assert "__shared__" not in code and "atomic" not in code
    # a world without damping takes the branch it took before: the schedule test and the launch are both behind damping_on()
    contacts = open(os.path.join(CSRC, "xpbd_world_contacts.cpp")).read()
    assert contacts.count("damping_on()") == 2 and contacts.count("launch_damping(") == 1
