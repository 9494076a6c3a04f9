"""The sweep-query ABI without a device: record layouts, the builder, the argument errors that need no world, and the
declarations in the header, the Rust text and the C++ host mirror."""
import os

import numpy as np

from constraint_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sweep_records_are_104_and_72_bytes():
    s, h = capi.SWEEP_DTYPE, capi.SWEEP_HIT_DTYPE
    assert s.itemsize == 104 and h.itemsize == 72
    assert [s.fields[k][1] for k in ("position", "rotation", "direction", "max_distance", "shape", "ignore_body", "mask", "reserved")] == \
        [0, 24, 56, 80, 88, 92, 96, 100]
    assert [h.fields[k][1] for k in ("body", "feature", "face", "reserved", "distance", "position", "normal")] == [0, 4, 8, 12, 16, 24, 48]
    assert (capi.SWEEP_BRUTE_FORCE, capi.SWEEP_MASKED, capi.SWEEP_INITIAL, capi.SWEEP_BRUTE_FORCE_SWEEPS) == (1, 2, 3, 8)
    assert capi.SWEEP_INITIAL not in (capi.FEATURE_FACE_A, capi.FEATURE_FACE_B, capi.FEATURE_EDGES)


def test_sweeps_builder_broadcasts_and_defaults():
    s = capi.sweeps([[0.0, 1.0, 2.0]], [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]], [1.0, 0.0, 0.0], 2, max_distance=[3.0, 4.0], ignore=[4, 7], mask=5)
    assert s.shape == (2,) and (s["position"] == [0.0, 1.0, 2.0]).all() and list(s["rotation"][1]) == [0.0, 1.0, 0.0, 0.0]
    assert (s["direction"] == [1.0, 0.0, 0.0]).all() and list(s["max_distance"]) == [3.0, 4.0]
    assert list(s["shape"]) == [2, 2] and list(s["ignore_body"]) == [4, 7] and list(s["mask"]) == [5, 5] and (s["reserved"] == 0).all()
    s = capi.sweeps(np.zeros((3, 3)), [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, -1.0], [0, 1, 2])
    assert s.shape == (3,) and (s["ignore_body"] == capi.NO_HIT).all() and (s["mask"] == 0xFFFFFFFF).all() and list(s["shape"]) == [0, 1, 2]
    assert np.isinf(s["max_distance"]).all()


def test_a_null_world_is_invalid_for_every_entry_point():
    L = capi.hip_lib()
    s = capi.sweeps([[0.0, 0.0, 0.0]], [1.0, 0.0, 0.0, 0.0], [1.0, 0.0, 0.0], 0)
    hits = np.zeros(2, dtype=capi.SWEEP_HIT_DTYPE)
    hits["body"] = 0xCDCDCDCD
    for fn in (L.xpbd_world_sweep, L.xpbd_world_sweep_device, L.xpbd_multi_world_sweep):
        assert fn(None, s.ctypes.data, 1, 0, hits.ctypes.data) == capi.E_INVALID
        assert b"NULL" in L.xpbd_last_error()
        assert fn(None, None, 0, 0, None) == capi.E_INVALID
    # (the remaining checks need a handle, and a handle needs a device: tests/test_gpu_sweep.py)
    assert (hits["body"] == 0xCDCDCDCD).all() and not hits["distance"].any()


def test_the_symbols_are_listed_and_exported():
    L = capi.hip_lib()
    for name in ("xpbd_world_sweep", "xpbd_world_sweep_device", "xpbd_multi_world_sweep"):
        assert name in capi.ABI_SYMBOLS and hasattr(L, name)
    assert L.xpbd_abi_version() == 2


def read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_the_declarations_are_in_the_header_the_rust_text_and_the_host_mirror():
    header = read("include", "xpbd.h")
    assert "Sweep queries (EXTENSION)" in header and header.index("Sweep queries (EXTENSION)") > header.index("xpbd_multi_world_overlap(")
    for text in ("#define XPBD_SWEEP_INITIAL 3u", "#define XPBD_SWEEP_BRUTE_FORCE 1u", "#define XPBD_SWEEP_MASKED 2u", "#define XPBD_SWEEP_BRUTE_FORCE_SWEEPS 8u",
                 "typedef struct xpbd_sweep {", "typedef struct xpbd_sweep_hit {", "xpbd_world_sweep(xpbd_world *w,", "xpbd_world_sweep_device(xpbd_world *w,",
                 "xpbd_multi_world_sweep(xpbd_multi_world *mw,"):
        assert text in header, text
    rust = read("constraint_solver_amd", "ffi", "xpbd_ffi.rs")
    for text in ("pub struct XpbdSweep {", "pub struct XpbdSweepHit {", "pub const XPBD_SWEEP_INITIAL: u32 = 3;", "pub fn xpbd_world_sweep(",
                 "pub fn xpbd_world_sweep_device(", "pub fn xpbd_multi_world_sweep("):
        assert text in rust, text
    host = read("constraint_solver_amd", "host", "constraint_solver.hpp")
    assert host.count("std::vector<xpbd_sweep_hit> sweep(const std::vector<xpbd_sweep> &sweeps") == 2
    assert "xpbd_world_sweep(w_" in host and "xpbd_multi_world_sweep(w_" in host
