"""Contact materials without a device: the record layout, the exported symbols, argument errors on a NULL world, the Rust
text, and the binding's conversion of plain coefficients into records."""
import ctypes as C
import os
import re

import numpy as np

from constraint_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["xpbd_world_set_materials", "xpbd_multi_world_set_materials"]


def test_material_record_is_sixteen_bytes_friction_then_reserved():
    dt = capi.MATERIAL_DTYPE
    assert dt.itemsize == 16
    assert dt.fields["friction"][1] == 0 and dt.fields["reserved"][1] == 8
    header = open(os.path.join(ROOT, "include", "xpbd.h")).read()
    body = re.search(r"typedef struct xpbd_material \{(.*?)\} xpbd_material;", header, re.S).group(1)
    assert re.findall(r"double\s+(\w+);", body) == ["friction", "reserved"]
    assert re.search(r"#define XPBD_ABI_VERSION 2u", header)


def test_new_symbols_are_exported_and_listed():
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libxpbd_hip.so"))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.ABI_SYMBOLS, name
    assert lib.xpbd_abi_version() == 2


def test_null_world_is_rejected_without_a_device():
    L = capi.hip_lib()
    m = np.zeros(3, dtype=capi.MATERIAL_DTYPE)
    assert L.xpbd_world_set_materials(None, None, 0, np.inf) == capi.E_INVALID
    assert b"NULL world" in L.xpbd_last_error()
    assert L.xpbd_world_set_materials(None, m.ctypes.data, 3, 0.5) == capi.E_INVALID
    assert L.xpbd_multi_world_set_materials(None, None, 0, np.inf) == capi.E_INVALID
    assert L.xpbd_multi_world_set_materials(None, m.ctypes.data, 3, 0.5) == capi.E_INVALID


def test_rust_text_declares_the_struct_and_both_calls():
    text = open(os.path.join(ROOT, "constraint_solver_amd", "ffi", "xpbd_ffi.rs")).read()
    body = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct XpbdMaterial \{(.*?)\}", text, re.S).group(1)
    assert re.findall(r"pub (\w+): f64", body) == ["friction", "reserved"]
    assert "XpbdMaterial { friction: f64::INFINITY, reserved: 0.0 }" in text
    for name, first in (("xpbd_world_set_materials", "w: *mut XpbdWorld"), ("xpbd_multi_world_set_materials", "mw: *mut XpbdMultiWorld")):
        m = re.search(r"pub fn %s\((.*?)\)\s*-> c_int;" % name, text, re.S)
        assert m, name
        args = [a.strip() for a in m.group(1).split(",")]
        assert args[0] == first and args[1] == "materials: *const XpbdMaterial" and args[3] == "ground_friction: f64"


def test_materials_accept_records_or_plain_coefficients():
    rec = capi._materials([0.0, 0.5, np.inf])
    assert rec.dtype == capi.MATERIAL_DTYPE and list(rec["friction"]) == [0.0, 0.5, np.inf] and not rec["reserved"].any()
    assert capi._materials(None) is None
    again = capi._materials(rec)
    assert again.dtype == capi.MATERIAL_DTYPE and again.tobytes() == rec.tobytes()
