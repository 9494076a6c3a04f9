"""Body population (include/xpbd.h, "Body POPULATION") without a device: the exported symbols, the struct-free signatures
against capi and the Rust text, the header's prose, and the argument errors that are returned before the device is touched.
(Without a device no world can be created, so the errors that need a live world -- no resident bodies, an index out of range,
a bad added body -- are in test_gpu_population.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from constraint_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["xpbd_world_remove_bodies", "xpbd_world_remove_bodies_device", "xpbd_world_add_bodies"]
# the header's parameters, as (C type, name)
SIGNATURES = {
    "xpbd_world_remove_bodies": [("xpbd_world *", "w"), ("const uint32_t *", "indices"), ("uint32_t", "n"), ("uint32_t *", "old_to_new"),
                                 ("uint32_t *", "joint_old_to_new"), ("uint32_t *", "n_bodies_out")],
    "xpbd_world_remove_bodies_device": [("xpbd_world *", "w"), ("const uint8_t *", "dev_remove"), ("uint32_t *", "dev_old_to_new"),
                                        ("uint32_t *", "joint_old_to_new"), ("uint32_t *", "n_bodies_out")],
    "xpbd_world_add_bodies": [("xpbd_world *", "w"), ("const xpbd_rigid *", "aos"), ("const uint32_t *", "shape_id"), ("uint32_t", "n_add"),
                              ("uint32_t *", "first_index_out")],
}
RUST_TYPES = {"xpbd_world *": "*mut XpbdWorld", "const uint32_t *": "*const u32", "uint32_t": "u32", "uint32_t *": "*mut u32",
              "const uint8_t *": "*const u8", "const xpbd_rigid *": "*const XpbdRigid"}


def header():
    return open(os.path.join(ROOT, "include", "xpbd.h")).read()


def test_new_symbols_are_exported_and_listed_and_the_abi_version_stays():
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libxpbd_hip.so"))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.ABI_SYMBOLS, name
    assert lib.xpbd_abi_version() == 2
    assert re.search(r"#define XPBD_ABI_VERSION 2u", header())


def test_header_signatures_match_capi_and_the_rust_text():
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    rust = open(os.path.join(ROOT, "constraint_solver_amd", "ffi", "xpbd_ffi.rs")).read()
    L = capi.hip_lib()
    for name, want in SIGNATURES.items():
        m = re.search(r"int\s+%s\((.*?)\);" % name, text, re.S)
        assert m, name
        params = [re.match(r"(.*?)(\w+)$", " ".join(p.split())).groups() for p in m.group(1).split(",")]
        assert [(t.strip(), n) for t, n in params] == want, name
        # capi: a pointer is passed as c_void_p (or a typed uint32 pointer), a count as c_uint32
        argtypes = getattr(L, name).argtypes
        assert len(argtypes) == len(want), name
        for (ctype, pname), got in zip(want, argtypes):
            if ctype == "uint32_t":
                assert got is C.c_uint32, (name, pname)
            else:
                assert got is C.c_void_p or got is C.POINTER(C.c_uint32), (name, pname)
        r = re.search(r"pub fn %s\((.*?)\)\s*-> c_int;" % name, rust, re.S)
        assert r, name
        rust_params = [tuple(x.strip() for x in p.split(":")) for p in " ".join(r.group(1).split()).split(",")]
        assert rust_params == [(pname, RUST_TYPES[ctype]) for ctype, pname in want], name


def test_header_section_says_what_travels_what_is_dropped_and_what_is_not_here():
    text = header()
    at = text.index("Body POPULATION (EXTENSION)")
    section = " ".join(text[at:text.index("int  xpbd_world_remove_bodies(", at)].replace(" * ", " ").split())
    for phrase in ("XPBD_NO_HIT", "relative order", "There are no handles", "38 doubles", "xpbd_world_set_external_wrench",
                   "collision-filter table", "friction table", "restitution table", "SLIDE", "joint_old_to_new",
                   "filter {~0u, ~0u}, friction +inf, restitution 0, no joints", "xpbd_world_history_length becomes 0",
                   "NO END events", "neighbour lists", "frame snapshot", "waits for completion", "removes the body once",
                   "changes nothing at all", "as xpbd_world_upload_bodies(.., 0) does", "leaves the previous population and settings in force",
                   "multi-GPU world", "per-call settings", "stable handles", "END events for removed bodies"):
        assert phrase in section, phrase


def test_null_world_is_rejected_without_a_device():
    L = capi.hip_lib()
    idx = np.arange(3, dtype=np.uint32)
    maps = np.full(8, 7, dtype=np.uint32)
    count = C.c_uint32(99)
    bodies = np.zeros((3, capi.RIGID_DOUBLES))
    flags = np.zeros(8, dtype=np.uint8)
    calls = {
        "xpbd_world_remove_bodies": lambda n: L.xpbd_world_remove_bodies(None, idx.ctypes.data, n, maps.ctypes.data, maps.ctypes.data, C.byref(count)),
        "xpbd_world_remove_bodies_device": lambda n: L.xpbd_world_remove_bodies_device(None, flags.ctypes.data, maps.ctypes.data, maps.ctypes.data,
                                                                                        C.byref(count)),
        "xpbd_world_add_bodies": lambda n: L.xpbd_world_add_bodies(None, bodies.ctypes.data, idx.ctypes.data, n, C.byref(count)),
    }
    assert sorted(calls) == sorted(NEW_SYMBOLS)
    for name, call in calls.items():
        for n in (3, 0):                                                 # (n == 0 is XPBD_OK only for a live world)
            assert call(n) == capi.E_INVALID, name
            message = L.xpbd_last_error()
            assert b"NULL world" in message and name.encode() in message, (name, message)
    assert count.value == 99 and (maps == 7).all()                       # nothing was written


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="this check is for the GPU-less build container")
def test_no_device_fails_loudly():
    with pytest.raises(capi.XpbdError) as e:
        capi.World()                                                     # there is no host path to fall back to
    assert e.value.code == capi.E_NO_DEVICE


def test_world_wrappers_exist_with_the_documented_signatures():
    import inspect
    assert list(inspect.signature(capi.World.remove_bodies).parameters) == ["self", "indices"]
    assert list(inspect.signature(capi.World.remove_bodies_device).parameters) == ["self", "dev_ptr", "dev_map_ptr"]
    assert inspect.signature(capi.World.remove_bodies_device).parameters["dev_map_ptr"].default is None
    assert list(inspect.signature(capi.World.add_bodies).parameters) == ["self", "bodies", "shape_id"]
