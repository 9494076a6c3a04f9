"""The overlap-query ABI without a device: record layouts, the query helper, the NULL-world error of every entry point and
the declarations in the header, the Rust text and the C++ host mirror."""
import os
import re

import numpy as np

from constraint_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_overlap_records_are_72_and_16_bytes():
    q, h = capi.OVERLAP_QUERY_DTYPE, capi.OVERLAP_HIT_DTYPE
    assert q.itemsize == 72 and h.itemsize == 16
    assert [q.fields[k][1] for k in ("position", "rotation", "shape", "ignore_body", "mask", "reserved")] == [0, 24, 56, 60, 64, 68]
    assert [h.fields[k][1] for k in ("body", "feature", "separation")] == [0, 4, 8]
    assert (capi.OVERLAP_BRUTE_FORCE, capi.OVERLAP_MASKED) == (1, 2)


def test_overlap_queries_helper_broadcasts_and_defaults():
    q = capi.overlap_queries([[0.0, 1.0, 2.0]], [[1.0, 0.0, 0.0, 0.0], [0.0, 1.0, 0.0, 0.0]], 2, ignore=[4, 7], mask=5)
    assert q.shape == (2,) and (q["position"] == [0.0, 1.0, 2.0]).all() and list(q["rotation"][1]) == [0.0, 1.0, 0.0, 0.0]
    assert list(q["shape"]) == [2, 2] and list(q["ignore_body"]) == [4, 7] and list(q["mask"]) == [5, 5] and (q["reserved"] == 0).all()
    q = capi.overlap_queries(np.zeros((3, 3)), [1.0, 0.0, 0.0, 0.0], [0, 1, 2])
    assert q.shape == (3,) and (q["ignore_body"] == capi.NO_HIT).all() and (q["mask"] == 0xFFFFFFFF).all() and list(q["shape"]) == [0, 1, 2]


def test_a_null_world_is_invalid_for_every_entry_point():
    L = capi.hip_lib()
    q = capi.overlap_queries([[0.0, 0.0, 0.0]], [1.0, 0.0, 0.0, 0.0], 0)
    offsets = np.full(2, 77, dtype=np.uint32)
    hits = np.zeros(4, dtype=capi.OVERLAP_HIT_DTYPE)
    total = capi.C.c_uint32(99)
    for fn in (L.xpbd_world_overlap, L.xpbd_multi_world_overlap):
        assert fn(None, q.ctypes.data, 1, 0, offsets.ctypes.data, hits.ctypes.data, 4, capi.C.byref(total)) == capi.E_INVALID
        assert b"NULL" in L.xpbd_last_error()
        assert fn(None, None, 0, 0, None, None, 0, None) == capi.E_INVALID
    assert L.xpbd_world_overlap_device(None, q.ctypes.data, 1, 0, offsets.ctypes.data, hits.ctypes.data, 4) == capi.E_INVALID
    assert b"NULL" in L.xpbd_last_error()
    # (the remaining checks need a handle, and a handle needs a device: tests/test_gpu_overlap.py)
    assert list(offsets) == [77, 77] and total.value == 99 and not hits["body"].any()


def test_the_symbols_are_listed_and_exported():
    L = capi.hip_lib()
    for name in ("xpbd_world_overlap", "xpbd_world_overlap_device", "xpbd_multi_world_overlap"):
        assert name in capi.ABI_SYMBOLS and hasattr(L, name)


def read(*path):
    with open(os.path.join(ROOT, *path)) as f:
        return f.read()


def test_the_declarations_are_in_the_header_the_rust_text_and_the_host_mirror():
    header = read("include", "xpbd.h")
    assert "Overlap queries (EXTENSION)" in header and header.index("Overlap queries (EXTENSION)") > header.index("xpbd_multi_world_raycast_masked(")
    for text in ("#define XPBD_OVERLAP_BRUTE_FORCE 1u", "#define XPBD_OVERLAP_MASKED      2u", "typedef struct xpbd_overlap_query {",
                 "typedef struct xpbd_overlap_hit {", "xpbd_world_overlap(xpbd_world *w,", "xpbd_world_overlap_device(xpbd_world *w,",
                 "xpbd_multi_world_overlap(xpbd_multi_world *mw,"):
        assert text in header, text
    rust = read("constraint_solver_amd", "ffi", "xpbd_ffi.rs")
    for text in ("pub struct XpbdOverlapQuery", "pub struct XpbdOverlapHit", "pub fn xpbd_world_overlap(", "pub fn xpbd_world_overlap_device(",
                 "pub fn xpbd_multi_world_overlap("):
        assert text in rust, text
    host = read("constraint_solver_amd", "host", "constraint_solver.hpp")
    assert host.count("> overlap(const std::vector<xpbd_overlap_query> &queries") == 2
    assert "xpbd_world_overlap(w_" in host and "xpbd_multi_world_overlap(w_" in host


def test_the_sort_stage_capi_names_is_the_kernels():
    m = re.search(r"constexpr uint32_t kOverlapSortStage = (\d+);", read("constraint_solver_amd", "csrc", "xpbd_query.h"))
    assert m and int(m.group(1)) == capi.OVERLAP_SORT_STAGE
