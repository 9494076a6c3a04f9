"""Mass edits without a device: the flags against the header, the exported symbols and their argument types, the Rust text and
the C++ mirror, what the header defines and says is out of scope, where the two older "Not here" notes went, and the one refusal
the library can show without a world (a NULL world).  Every other refusal is the work of the host-only checks:
tests/test_mass_edit_checks_standalone.py."""
import ctypes as C
import os
import re

import numpy as np

import mass_edit_model as mm
from constraint_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "constraint_solver_amd", "csrc")
SETTERS = ["xpbd_world_set_mass_properties", "xpbd_world_set_mass_properties_device"]
NEW_SYMBOLS = SETTERS + ["xpbd_world_get_mass_properties"]


def header():
    return open(os.path.join(ROOT, "include", "xpbd.h")).read()


def flat(text):
    return re.sub(r"\s*\n \*\s*", " ", text)


def section():
    text = flat(header())
    return text[text.index("MASS properties of resident bodies (EXTENSION)"):text.index("Body POPULATION (EXTENSION)")]


def test_flags_are_the_headers():
    for name, value in (("INVERSE", 0), ("DIRECT", 1), ("KEEP_FRAME", 0x100)):
        assert int(re.search(r"#define XPBD_MASS_%s\s+(\w+)u" % name, header()).group(1), 0) == value == getattr(capi, "MASS_" + name) == getattr(mm, name)
    assert capi.MASS_DOUBLES == 13 == len(mm.MASS_COLUMNS)
    assert [capi.RIGID_FIELDS[f] for f in ("inverse_mass", "inverse_inertia", "center_of_mass")] == [(0, 1), (1, 9), (28, 3)]


def test_new_symbols_are_exported_listed_and_typed():
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libxpbd_hip.so"))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.ABI_SYMBOLS, name
    L = capi.hip_lib()
    p, u = C.c_void_p, C.c_uint32
    assert L.xpbd_world_set_mass_properties.argtypes == [p, p, u, p, u]
    assert L.xpbd_world_set_mass_properties_device.argtypes == [p, p, u, p, u]
    assert L.xpbd_world_get_mass_properties.argtypes == [p, p, u, p]
    text = header()
    assert re.search(r"int\s+xpbd_world_set_mass_properties\(xpbd_world \*w, const uint32_t \*indices, uint32_t n, const double \*rows[^,]*, uint32_t flags\);", text)
    assert re.search(r"int\s+xpbd_world_set_mass_properties_device\(xpbd_world \*w, const uint32_t \*dev_indices, uint32_t n, const double \*dev_rows, uint32_t flags\);", text)
    assert re.search(r"int\s+xpbd_world_get_mass_properties\(xpbd_world \*w, const uint32_t \*indices, uint32_t n, double \*rows.*?\);", text)


def test_the_header_defines_the_edit_and_names_what_is_out_of_scope():
    text = section()
    for words in ("inverse_mass = 1.0 / mass", "det == 0.0 is singular", "cross(m.y, m.z) / det", "d = com' - com", "r = q * d",
                  "position' = position + (r - d)", "velocity' = velocity + cross(angular_velocity, r)", "no dynamic double is touched",
                  "steps bit for bit like a fresh world", "XPBD_E_SINGULAR_INERTIA", "clear its entry first", "one entry wins whole",
                  "STAYS after xpbd_world_history_restore", "xpbd_world_contacts_begin again", "per-body records", "wakes everybody",
                  "from BEFORE the edit", "returns rows in the INVERSE layout"):
        assert words in text, words
    not_here = text[text.index("Not here:"):]
    for words in ("multi-GPU world", "shadow copy", "per-shape table again", "density"):
        assert words in not_here, words


def test_the_two_older_notes_moved():
    text = flat(header())
    edits = text[text.index("Not here: xpbd_multi_world_set_dynamics"):]
    edits = edits[:edits.index("----")]
    assert "changing the mass properties of resident bodies" not in edits and '"MASS properties of resident bodies"' in edits
    kinematic = text[text.index("KINEMATIC bodies (EXTENSION)"):text.index("typedef struct xpbd_kinematic")]
    assert "cannot change yet" not in kinematic and "freeze it first" in kinematic
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Mass edits" in design and "per-body records until the next upload" in design
    for name in ("README.md", "INTEGRATION.md"):
        assert "xpbd_world_set_mass_properties" in open(os.path.join(ROOT, name)).read(), name


def test_rust_text_and_cpp_mirror_bind_the_calls():
    text = open(os.path.join(ROOT, "constraint_solver_amd", "ffi", "xpbd_ffi.rs")).read()
    for name, value in (("INVERSE", "0"), ("DIRECT", "1"), ("KEEP_FRAME", "0x100")):
        assert re.search(r"pub const XPBD_MASS_%s: u32 = %s;" % (name, value), text), name
    for name in SETTERS:
        args = [a.strip() for a in re.search(r"pub fn %s\((.*?)\)\s*-> c_int;" % name, text, re.S).group(1).split(",")]
        assert args[0] == "w: *mut XpbdWorld" and args[2] == "n: u32" and args[4] == "flags: u32" and args[3].endswith("*const f64"), name
    assert re.search(r"pub fn xpbd_world_get_mass_properties\(w: \*mut XpbdWorld, indices: \*const u32, n: u32, rows: \*mut f64\) -> c_int;", text)
    host = open(os.path.join(ROOT, "constraint_solver_amd", "host", "constraint_solver.hpp")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"check\(%s\(w_, " % name, host), name


def test_null_world_is_rejected_without_a_device():
    L = capi.hip_lib()
    idx, rows = np.zeros(1, dtype=np.uint32), np.zeros(13)
    calls = {
        "xpbd_world_set_mass_properties": lambda n: (idx.ctypes.data, n, rows.ctypes.data, 0),
        "xpbd_world_set_mass_properties_device": lambda n: (idx.ctypes.data, n, rows.ctypes.data, 0),
        "xpbd_world_get_mass_properties": lambda n: (idx.ctypes.data, n, rows.ctypes.data),
    }
    for name, args in calls.items():
        for n in (1, 0):                                                      # ... also with n == 0, which a live world accepts
            assert getattr(L, name)(None, *args(n)) == capi.E_INVALID, name
            message = L.xpbd_last_error()
            assert b"NULL world" in message and name.encode() in message, (name, message)


def test_the_unit_is_listed_where_the_others_are_and_uses_neither_lds_nor_atomics():
    build = open(os.path.join(ROOT, "constraint_solver_amd", "_build.py")).read()
    assert '"xpbd_mass_edit.hip"' in build and "-ffp-contract=off" in build
    hip = open(os.path.join(CSRC, "xpbd_mass_edit.hip")).read()
    for kernel in ("k_set_mass", "k_get_mass"):
        assert "__global__ void __launch_bounds__(kBlock) %s(" % kernel in hip, kernel
    assert "__shared__" not in hip and "atomic" not in hip.replace("no atomics", "") and "asm" not in hip
    assert "resolve_mass_row(" in hip and "resolve_mass_row(" in open(os.path.join(CSRC, "xpbd_checks.cpp")).read()    # one predicate
