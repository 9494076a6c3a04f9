"""Sensor bodies without a device: the record layout against the header, the exported symbols, the Rust text and the C++ mirror,
what the header says is out of scope, and the one refusal the library can show without a world (a NULL world).  Every other
refusal is the work of the host-only checks: tests/test_sensor_checks_standalone.py."""
import ctypes as C
import os
import re

import numpy as np

from constraint_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "constraint_solver_amd", "csrc")
CALLS = ["xpbd_world_set_sensors", "xpbd_world_get_sensors", "xpbd_world_sensor_overlaps", "xpbd_world_sensor_overlaps_device"]
NEW_SYMBOLS = CALLS + ["xpbd_world_sensor_count"]
FIELDS = [("body", 0), ("pair", 4)]


def header():
    return open(os.path.join(ROOT, "include", "xpbd.h")).read()


def section():
    text = re.sub(r"\s*\n \*\s*", " ", header())
    return text[text.index("SENSOR bodies (EXTENSION)"):text.index("typedef struct xpbd_sensor_hit")]


def test_hit_is_eight_bytes_with_the_headers_fields():
    assert capi.SENSOR_HIT_DTYPE.itemsize == 8
    for name, at in FIELDS:
        assert capi.SENSOR_HIT_DTYPE.fields[name][1] == at and capi.SENSOR_HIT_DTYPE.fields[name][0] == np.dtype("<u4"), name
    m = re.search(r"typedef struct xpbd_sensor_hit \{\s*/\* (\d+) bytes \*/(.*?)\} xpbd_sensor_hit;", header(), re.S)
    assert int(m.group(1)) == 8
    body = re.sub(r"/\*.*?\*/", "", m.group(2), flags=re.S)
    assert re.findall(r"uint32_t\s+(\w+);", body) == [name for name, _ in FIELDS]


def test_the_header_defines_the_semantics_and_names_what_is_out_of_scope():
    text = section()
    for words in ("at least one sensor end", "see a code of 0", "BIT FOR BIT", "{group 0, mask 0}", "exclude sensor pairs", "pair count includes",
                  "Sensor-sensor pairs are reported too", "not contact edges", "never inert", "no END event at sleep",
                  "MOVING kinematic sensor wakes what it shares a pair with", "xpbd_world_upload_bodies clears the table", "new bodies are not sensors",
                  "History push and restore do not carry the table", "wakes everybody", "enqueued before", "the other bits stay reserved",
                  "XPBD_E_CAPACITY is returned with the first `cap` filled", "waits only when its scratch has to grow",
                  "exactly when xpbd_world_contact_report_counts is XPBD_E_INVALID"):
        assert words in text, words
    not_here = text[text.index("Not here:"):]
    for words in ("multi-GPU world", "per-sensor filter beyond group / mask"):
        assert words in not_here, words
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "Sensor bodies" in design
    assert "xpbd_world_set_sensors" in open(os.path.join(ROOT, "README.md")).read()


def test_new_symbols_are_exported_and_listed():
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libxpbd_hip.so"))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.ABI_SYMBOLS, name
    for method in ("set_sensors", "get_sensors", "sensor_count", "sensor_overlaps", "sensor_overlaps_device"):
        assert callable(getattr(capi.World, method)), method


def test_rust_text_and_cpp_mirror_bind_the_calls():
    text = open(os.path.join(ROOT, "constraint_solver_amd", "ffi", "xpbd_ffi.rs")).read()
    body = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct XpbdSensorHit \{(.*?)\}", text, re.S).group(1)
    assert re.findall(r"pub (\w+): ([\w\[\]; ]+),", body) == [("body", "u32"), ("pair", "u32")]
    for name in CALLS:
        args = [a.strip() for a in re.search(r"pub fn %s\((.*?)\)\s*-> c_int;" % name, text, re.S).group(1).split(",")]
        assert args[0] == "w: *mut XpbdWorld", name
    assert re.search(r"pub fn xpbd_world_sensor_count\(w: \*const XpbdWorld\) -> u32;", text)
    host = open(os.path.join(ROOT, "constraint_solver_amd", "host", "constraint_solver.hpp")).read()
    for name in CALLS:
        assert re.search(r"%s\(w_, " % name, host), name
    assert "xpbd_world_sensor_count(w_)" in host


def test_null_world_is_rejected_without_a_device():
    L = capi.hip_lib()
    flags, idx, n_out = np.zeros(4, dtype=np.uint8), np.zeros(4, dtype=np.uint32), C.c_uint32(0)
    hits = np.zeros(4, dtype=capi.SENSOR_HIT_DTYPE)
    calls = {
        "xpbd_world_set_sensors": (flags.ctypes.data, 4),
        "xpbd_world_get_sensors": (flags.ctypes.data, 4),
        "xpbd_world_sensor_overlaps": (idx.ctypes.data, idx.ctypes.data, hits.ctypes.data, 4, C.byref(n_out)),
        "xpbd_world_sensor_overlaps_device": (idx.ctypes.data, idx.ctypes.data, hits.ctypes.data, 4),
    }
    for name, args in calls.items():
        assert getattr(L, name)(None, *args) == capi.E_INVALID, name
        message = L.xpbd_last_error()
        assert b"NULL world" in message and name.encode() in message, (name, message)
    assert L.xpbd_world_set_sensors(None, None, 0) == capi.E_INVALID          # ... also the clearing call, which a live world accepts
    assert L.xpbd_world_sensor_count(None) == 0


def test_the_units_are_listed_where_the_others_are():
    build = open(os.path.join(ROOT, "constraint_solver_amd", "_build.py")).read()
    assert '"xpbd_sensors.hip"' in build and '"xpbd_world_sensors.cpp"' in build
    hip = open(os.path.join(CSRC, "xpbd_sensors.hip")).read()
    for kernel in ("k_sensor_mask_codes", "k_sensor_solid_flag", "k_sensor_solid_write", "k_sensor_not_inert", "k_sensor_list", "k_sensor_gather",
                   "k_sensor_overlaps"):
        assert "__global__ void __launch_bounds__(kBlock) %s(" % kernel in hip, kernel
    code = re.sub(r"//.*", "", hip)
    assert "__shared__" not in code and "atomic" not in code and "double" not in code and "float" not in code


def test_islands_and_sleeping_take_their_edges_from_the_one_helper():
    """Islands::enqueue and Sleep::frame_end no longer compact the report's keys themselves."""
    for name in ("xpbd_world_islands.cpp", "xpbd_world_sleep.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "contact_edge_keys(w, " in text and "compact_keys" not in text, name
