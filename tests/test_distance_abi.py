"""The distance-query ABI without a device: record layouts, the builder, the argument errors that need no world, and the
declarations in the header, the Rust text and the C++ host mirror."""
import os

import numpy as np

from constraint_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_distance_records_are_80_and_96_bytes():
    q, h = capi.DISTANCE_QUERY_DTYPE, capi.DISTANCE_HIT_DTYPE
    assert q.itemsize == 80 and h.itemsize == 96
    assert [q.fields[k][1] for k in ("position", "rotation", "max_distance", "shape", "ignore_body", "mask", "reserved")] == [0, 24, 56, 64, 68, 72, 76]
    assert [h.fields[k][1] for k in ("body", "feature", "index_a", "index_b", "distance", "point_a", "point_b", "normal")] == [0, 4, 8, 12, 16, 24, 48, 72]
    assert (capi.DISTANCE_BRUTE_FORCE, capi.DISTANCE_MASKED, capi.DISTANCE_OVERLAP, capi.DISTANCE_BRUTE_FORCE_QUERIES) == (1, 2, 3, 8)
    assert capi.DISTANCE_POINT == 0xFFFFFFFF
    assert capi.DISTANCE_OVERLAP not in (capi.FEATURE_FACE_A, capi.FEATURE_FACE_B, capi.FEATURE_EDGES)


def test_distances_builder_broadcasts_and_defaults():
    q = capi.distances([[0.0, 1.0, 2.0]], [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]], 2, max_distance=[3.0, 4.0], ignore=[4, 7], mask=5)
    assert q.shape == (2,) and (q["position"] == [0.0, 1.0, 2.0]).all() and list(q["rotation"][1]) == [0.0, 1.0, 0.0, 0.0]
    assert list(q["max_distance"]) == [3.0, 4.0]
    assert list(q["shape"]) == [2, 2] and list(q["ignore_body"]) == [4, 7] and list(q["mask"]) == [5, 5] and (q["reserved"] == 0).all()
    q = capi.distances(np.zeros((3, 3)))                                     # points, as far as it takes, nothing ignored
    assert q.shape == (3,) and (q["shape"] == capi.DISTANCE_POINT).all() and (q["rotation"] == [1.0, 0.0, 0.0, 0.0]).all()
    assert (q["ignore_body"] == capi.NO_HIT).all() and (q["mask"] == 0xFFFFFFFF).all() and np.isinf(q["max_distance"]).all()
    q = capi.distances(np.zeros((3, 3)), shape=[0, 1, 2], max_distance=0.5)
    assert list(q["shape"]) == [0, 1, 2] and (q["max_distance"] == 0.5).all()


def test_a_null_world_is_invalid_for_every_entry_point():
    L = capi.hip_lib()
    q = capi.distances([[0.0, 0.0, 0.0]])
    hits = np.zeros(2, dtype=capi.DISTANCE_HIT_DTYPE)
    hits["body"] = 0xCDCDCDCD
    for fn in (L.xpbd_world_distance, L.xpbd_world_distance_device, L.xpbd_multi_world_distance):
        assert fn(None, q.ctypes.data, 1, 0, hits.ctypes.data) == capi.E_INVALID
        assert b"NULL" in L.xpbd_last_error()
        assert fn(None, None, 0, 0, None) == capi.E_INVALID
    # (the remaining checks need a handle, and a handle needs a device: tests/test_gpu_distance.py)
    assert (hits["body"] == 0xCDCDCDCD).all() and not hits["distance"].any()


def test_the_symbols_are_listed_and_exported():
    L = capi.hip_lib()
    for name in ("xpbd_world_distance", "xpbd_world_distance_device", "xpbd_multi_world_distance"):
        assert name in capi.ABI_SYMBOLS and hasattr(L, name)
    assert L.xpbd_abi_version() == 2


def read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_the_declarations_are_in_the_header_the_rust_text_and_the_host_mirror():
    header = read("include", "xpbd.h")
    assert "Distance queries (EXTENSION)" in header and header.index("Distance queries (EXTENSION)") > header.index("xpbd_multi_world_sweep(")
    for text in ("#define XPBD_DISTANCE_BRUTE_FORCE 1u", "#define XPBD_DISTANCE_MASKED      2u", "#define XPBD_DISTANCE_OVERLAP     3u",
                 "#define XPBD_DISTANCE_POINT       0xFFFFFFFFu", "#define XPBD_DISTANCE_BRUTE_FORCE_QUERIES 8u",
                 "typedef struct xpbd_distance_query {", "typedef struct xpbd_distance_hit {", "xpbd_world_distance(xpbd_world *w,",
                 "xpbd_world_distance_device(xpbd_world *w,", "xpbd_multi_world_distance(xpbd_multi_world *mw,"):
        assert text in header, text
    rust = read("constraint_solver_amd", "ffi", "xpbd_ffi.rs")
    for text in ("pub struct XpbdDistanceQuery {", "pub struct XpbdDistanceHit {", "pub const XPBD_DISTANCE_OVERLAP: u32 = 3;",
                 "pub const XPBD_DISTANCE_POINT: u32 = 0xFFFF_FFFF;", "pub fn xpbd_world_distance(", "pub fn xpbd_world_distance_device(",
                 "pub fn xpbd_multi_world_distance("):
        assert text in rust, text
    host = read("constraint_solver_amd", "host", "constraint_solver.hpp")
    assert host.count("std::vector<xpbd_distance_hit> distance(const std::vector<xpbd_distance_query> &queries") == 2
    assert "xpbd_world_distance(w_" in host and "xpbd_multi_world_distance(w_" in host
