"""Body edits without a device: the record layout, the exported symbols, the Rust text, and the argument errors that are
returned before any device work.  (Without a device no world can be created, so the errors that need a live world -- no
resident bodies, indices out of range or listed twice, unknown flags, non-finite values -- are in test_gpu_body_edits.py.)"""
import ctypes as C
import os
import re

import numpy as np

from constraint_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["xpbd_world_set_external_wrench", "xpbd_world_set_external_wrench_device", "xpbd_world_apply_impulses",
               "xpbd_world_apply_impulses_device", "xpbd_world_set_dynamics", "xpbd_world_get_dynamics",
               "xpbd_multi_world_set_external_wrench", "xpbd_multi_world_apply_impulses"]
FIELDS = [("body", 0), ("flags", 4), ("impulse", 8), ("point", 32), ("angular_impulse", 56)]


def test_impulse_record_is_eighty_bytes_with_the_headers_fields():
    assert C.sizeof(capi.Impulse) == 80 and capi.IMPULSE_DTYPE.itemsize == 80
    for name, at in FIELDS:
        assert getattr(capi.Impulse, name).offset == at, name
        assert capi.IMPULSE_DTYPE.fields[name][1] == at, name
    header = open(os.path.join(ROOT, "include", "xpbd.h")).read()
    body = re.search(r"typedef struct xpbd_impulse \{(.*?)\} xpbd_impulse;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)(?:\[3\])?[,;]", body) == ["body", "flags", "impulse", "point", "angular_impulse"]
    assert re.search(r"#define XPBD_IMPULSE_AT_POINT\s+0u", header) and re.search(r"#define XPBD_IMPULSE_AT_CENTRE\s+1u", header)
    assert (capi.IMPULSE_AT_POINT, capi.IMPULSE_AT_CENTRE) == (0, 1)
    assert re.search(r"#define XPBD_ABI_VERSION 2u", header)


def test_new_symbols_are_exported_and_listed():
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libxpbd_hip.so"))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.ABI_SYMBOLS, name
    assert lib.xpbd_abi_version() == 2


def test_rust_text_declares_the_struct_and_all_eight_calls():
    text = open(os.path.join(ROOT, "constraint_solver_amd", "ffi", "xpbd_ffi.rs")).read()
    body = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct XpbdImpulse \{(.*?)\}", text, re.S).group(1)
    assert re.findall(r"pub (\w+): ([^,]+),", body) == [("body", "u32"), ("flags", "u32"), ("impulse", "[f64; 3]"), ("point", "[f64; 3]"),
                                                        ("angular_impulse", "[f64; 3]")]
    assert "pub const XPBD_IMPULSE_AT_CENTRE: u32 = 1;" in text and "pub const XPBD_IMPULSE_AT_POINT: u32 = 0;" in text
    for name in NEW_SYMBOLS:
        m = re.search(r"pub fn %s\((.*?)\)\s*-> c_int;" % name, text, re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert args[0] == ("mw: *mut XpbdMultiWorld" if "multi" in name else "w: *mut XpbdWorld"), name
        if "impulses" in name:
            assert args[1].endswith("*const XpbdImpulse") and args[2] == "n: u32", name
        else:
            assert args[1].endswith("indices: *const u32") and args[2] == "n: u32", name
    assert "rows: *mut f64" in re.search(r"pub fn xpbd_world_get_dynamics\((.*?)\)", text, re.S).group(1)


def test_null_world_is_rejected_without_a_device():
    L = capi.hip_lib()
    idx = np.arange(3, dtype=np.uint32)
    xyz = np.zeros((3, 3))
    rows = np.zeros((3, 13))
    imp = np.zeros(3, dtype=capi.IMPULSE_DTYPE)
    calls = {
        "xpbd_world_set_external_wrench": (idx.ctypes.data, 3, xyz.ctypes.data, xyz.ctypes.data),
        "xpbd_world_set_external_wrench_device": (idx.ctypes.data, 3, xyz.ctypes.data, xyz.ctypes.data),
        "xpbd_world_apply_impulses": (imp.ctypes.data, 3),
        "xpbd_world_apply_impulses_device": (imp.ctypes.data, 3),
        "xpbd_world_set_dynamics": (idx.ctypes.data, 3, rows.ctypes.data),
        "xpbd_world_get_dynamics": (idx.ctypes.data, 3, rows.ctypes.data),
        "xpbd_multi_world_set_external_wrench": (idx.ctypes.data, 3, xyz.ctypes.data, xyz.ctypes.data),
        "xpbd_multi_world_apply_impulses": (imp.ctypes.data, 3),
    }
    assert sorted(calls) == sorted(NEW_SYMBOLS)
    for name, args in calls.items():
        assert getattr(L, name)(None, *args) == capi.E_INVALID, name
        message = L.xpbd_last_error()
        assert b"NULL world" in message and name.encode() in message, (name, message)
        # ... also with n == 0, which only a live world answers with XPBD_OK
        empty = tuple(0 if isinstance(a, int) and a == 3 else a for a in args)
        assert getattr(L, name)(None, *empty) == capi.E_INVALID, name


def test_impulses_helper_builds_records():
    rec = capi.impulses([4, 2], [[1.0, 2.0, 3.0]], point=[[0.0, 0.5, 1.0], [1.0, 1.0, 1.0]], angular_impulse=[0.0, 0.0, 2.0])
    assert rec.dtype == capi.IMPULSE_DTYPE and list(rec["body"]) == [4, 2] and not rec["flags"].any()
    assert rec["impulse"].tolist() == [[1.0, 2.0, 3.0]] * 2 and rec["point"].tolist() == [[0.0, 0.5, 1.0], [1.0, 1.0, 1.0]]
    assert rec["angular_impulse"].tolist() == [[0.0, 0.0, 2.0]] * 2
    centre = capi.impulses(7, [0.0, 0.0, 1.0])
    assert centre["flags"].tolist() == [capi.IMPULSE_AT_CENTRE] and not centre["point"].any()
