"""Collision filters without a device: the record layout, the exported symbols, argument errors on a NULL world, and the
symmetry of the filtered lists the model (tests/collision_filter_model.py) derives."""
import ctypes as C
import os
import re

import numpy as np

import collision_filter_model as fm
from constraint_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["xpbd_world_set_collision_filters", "xpbd_multi_world_set_collision_filters", "xpbd_world_raycast_masked",
               "xpbd_world_raycast_masked_device", "xpbd_multi_world_raycast_masked"]


def test_filter_record_is_eight_bytes_group_then_mask():
    dt = capi.COLLISION_FILTER_DTYPE
    assert dt.itemsize == 8
    assert dt.fields["group"][1] == 0 and dt.fields["mask"][1] == 4
    header = open(os.path.join(ROOT, "include", "xpbd.h")).read()
    body = re.search(r"typedef struct xpbd_collision_filter \{(.*?)\} xpbd_collision_filter;", header, re.S).group(1)
    assert re.findall(r"uint32_t\s+(\w+);", body) == ["group", "mask"]
    assert re.search(r"#define XPBD_FILTER_JOINTED 1u", header)
    assert capi.FILTER_JOINTED == 1


def test_new_symbols_are_exported_and_listed():
    lib = C.CDLL(os.path.join(capi.LIB_DIR, "libxpbd_hip.so"))
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in capi.ABI_SYMBOLS, name


def test_null_world_is_rejected_without_a_device():
    L = capi.hip_lib()
    f = np.zeros(3, dtype=capi.COLLISION_FILTER_DTYPE)
    assert L.xpbd_world_set_collision_filters(None, None, 0, 0) == capi.E_INVALID
    assert b"NULL world" in L.xpbd_last_error()
    assert L.xpbd_world_set_collision_filters(None, f.ctypes.data, 3, capi.FILTER_JOINTED) == capi.E_INVALID
    assert L.xpbd_multi_world_set_collision_filters(None, None, 0, 0) == capi.E_INVALID
    hits = np.zeros(1, dtype=capi.RAY_HIT_DTYPE)
    rays = capi.rays([0.0, 0.0, 5.0], [0.0, 0.0, -1.0])
    assert L.xpbd_world_raycast_masked(None, rays.ctypes.data, 1, 0, 1, hits.ctypes.data) == capi.E_INVALID
    assert L.xpbd_world_raycast_masked_device(None, None, 0, 0, 1, None) == capi.E_INVALID
    assert L.xpbd_multi_world_raycast_masked(None, rays.ctypes.data, 1, 0, 1, hits.ctypes.data) == capi.E_INVALID


def random_symmetric_lists(rng, n, p):
    adj = np.triu(rng.random((n, n)) < p, 1)
    adj = adj | adj.T
    off = np.concatenate([[0], np.cumsum(adj.sum(axis=1))]).astype(np.uint32)
    nb = np.concatenate([np.flatnonzero(adj[i]) for i in range(n)]).astype(np.uint32)
    return off, nb


def test_model_lists_are_symmetric_and_follow_the_rule():
    rng = np.random.default_rng(7)
    n = 120
    off, nb = random_symmetric_lists(rng, n, 0.15)
    filters = np.zeros(n, dtype=capi.COLLISION_FILTER_DTYPE)
    filters["group"] = 1 << rng.integers(0, 4, n)
    filters["mask"] = rng.integers(0, 16, n)
    joints = np.zeros(40, dtype=capi.JOINT_DTYPE)
    joints["body_a"] = rng.integers(0, n // 2, 40)
    joints["body_b"] = joints["body_a"] + 1 + rng.integers(0, n // 2, 40)
    for jointed in (False, True):
        f_off, f_nb = fm.filter_lists(off, nb, filters, joints, jointed)
        assert fm.is_symmetric(f_off, f_nb)
        assert 0 < len(f_nb) < len(nb)
        joined = fm.joined_pairs(joints)
        for i in range(n):
            mine = set(f_nb[f_off[i]:f_off[i + 1]].tolist())
            for j in nb[off[i]:off[i + 1]].tolist():
                keep = ((filters["group"][i] & filters["mask"][j]) != 0 and (filters["group"][j] & filters["mask"][i]) != 0
                        and not (jointed and (min(i, j), max(i, j)) in joined))
                assert (j in mine) == keep
    # no filters, no joints: the lists stay as they are
    same_off, same_nb = fm.filter_lists(off, nb)
    assert np.array_equal(same_off, off) and np.array_equal(same_nb, nb)


def test_filters_accept_records_or_group_mask_rows():
    rows = np.array([[1, 2], [3, 4]], dtype=np.uint32)
    rec = capi._filters(rows)
    assert rec.dtype == capi.COLLISION_FILTER_DTYPE and list(rec["group"]) == [1, 3] and list(rec["mask"]) == [2, 4]
    assert capi._filters(None) is None
    assert capi._filters(rec) is rec or np.array_equal(capi._filters(rec), rec)
