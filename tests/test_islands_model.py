"""The independent model of the contact islands (islands_model.py) against hand-written answers for tiny graphs, and the
layout of xpbd_island in the binding and the model against include/xpbd.h."""
import os
import re

import numpy as np

import islands_model as im
from constraint_solver_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = im.ISLAND_NONE


def bodies(n, fixed=(), heavy=(), velocity=None, angular=None):
    """n unit bodies; `fixed`: inverse mass and inverse inertia all zero; `heavy`: zero inverse mass but a body that can turn."""
    b = np.zeros((n, 38))
    b[:, 0] = 1.0
    b[:, [1, 5, 9]] = 6.0
    b[:, 34] = 1.0
    for i in fixed:
        b[i, 0:10] = 0.0
    for i in heavy:
        b[i, 0] = 0.0
    for i, v in (velocity or {}).items():
        b[i, 22:25] = v
    for i, v in (angular or {}).items():
        b[i, 25:28] = v
    return b


def edges(*ab):
    return np.array(ab, dtype=np.uint32).reshape(-1, 2)


def rows(records):
    """(first_body, n_bodies, n_pairs, n_joints, n_anchors, n_grounded) per island."""
    return [tuple(int(r[f]) for f in ("first_body", "n_bodies", "n_pairs", "n_joints", "n_anchors", "n_grounded")) for r in records]


def no_masks(n):
    return np.zeros(n, dtype=np.uint32)


def test_fixed_hub_with_three_leaves_is_three_islands_with_one_anchor_each():
    of, rec = im.islands(bodies(4, fixed=[0]), edges((0, 1), (0, 2), (0, 3)), None, no_masks(4))
    assert of.tolist() == [NONE, 0, 1, 2]
    assert rows(rec) == [(1, 1, 0, 0, 1, 0), (2, 1, 0, 0, 1, 0), (3, 1, 0, 0, 1, 0)]


def test_a_free_hub_with_three_leaves_is_one_island():
    of, rec = im.islands(bodies(4), edges((0, 1), (0, 2)), edges((3, 0)), no_masks(4))
    assert of.tolist() == [0, 0, 0, 0]
    assert rows(rec) == [(0, 4, 2, 1, 0, 0)]


def test_two_fixed_bodies_joined_to_each_other_are_ignored():
    of, rec = im.islands(bodies(3, fixed=[0, 1]), edges((0, 1)), edges((1, 0)), no_masks(3))
    assert of.tolist() == [NONE, NONE, 0]
    assert rows(rec) == [(2, 1, 0, 0, 0, 0)]


def test_a_world_of_fixed_bodies_has_no_islands():
    of, rec = im.islands(bodies(2, fixed=[0, 1]), edges((0, 1)), None, no_masks(2))
    assert of.tolist() == [NONE, NONE] and len(rec) == 0


def test_a_self_contained_triangle():
    of, rec = im.islands(bodies(5), edges((1, 2), (2, 4)), edges((4, 1)), no_masks(5))
    assert of.tolist() == [0, 1, 1, 2, 1]
    assert rows(rec) == [(0, 1, 0, 0, 0, 0), (1, 3, 2, 1, 0, 0), (3, 1, 0, 0, 0, 0)]


def test_an_isolated_body_is_an_island_of_one():
    of, rec = im.islands(bodies(1), None, None, np.array([5], dtype=np.uint32))
    assert of.tolist() == [0] and rows(rec) == [(0, 1, 0, 0, 0, 1)]


def test_islands_are_numbered_by_their_smallest_member():
    of, rec = im.islands(bodies(6), edges((3, 5), (0, 4)), edges((2, 1)), no_masks(6))
    assert of.tolist() == [0, 1, 1, 2, 0, 2]
    assert [int(r["first_body"]) for r in rec] == [0, 1, 3]


def test_zero_inverse_mass_with_inertia_is_not_fixed():
    of, rec = im.islands(bodies(3, heavy=[0]), edges((0, 1), (0, 2)), None, no_masks(3))
    assert of.tolist() == [0, 0, 0] and rows(rec) == [(0, 3, 2, 0, 0, 0)]


def test_both_flags_one_at_a_time():
    b, pairs, joints = bodies(5, fixed=[4]), edges((0, 1), (1, 4)), edges((1, 2), (3, 4), (2, 1))
    of, rec = im.islands(b, pairs, joints, no_masks(5))
    assert of.tolist() == [0, 0, 0, 1, NONE] and rows(rec) == [(0, 3, 1, 2, 1, 0), (3, 1, 0, 0, 1, 0)]
    of, rec = im.islands(b, pairs, joints, no_masks(5), im.NO_JOINTS)
    assert of.tolist() == [0, 0, 1, 2, NONE] and rows(rec) == [(0, 2, 1, 0, 1, 0), (2, 1, 0, 0, 0, 0), (3, 1, 0, 0, 0, 0)]
    of, rec = im.islands(b, pairs, joints, no_masks(5), im.NO_CONTACTS)
    assert of.tolist() == [0, 1, 1, 2, NONE] and rows(rec) == [(0, 1, 0, 0, 0, 0), (1, 2, 0, 2, 0, 0), (3, 1, 0, 0, 1, 0)]


def test_duplicate_joints_count_twice_and_connect_once():
    of, rec = im.islands(bodies(3), None, edges((0, 2), (2, 0), (0, 2)), no_masks(3))
    assert of.tolist() == [0, 1, 0] and rows(rec) == [(0, 2, 0, 3, 0, 0), (1, 1, 0, 0, 0, 0)]


def test_grounded_members_and_the_maxima():
    b = bodies(4, velocity={0: (3.0, 0.0, -4.0), 1: (0.0, -6.0, 0.0), 3: (1.0, 1.0, 1.0)}, angular={1: (0.0, 0.0, -2.0)})
    of, rec = im.islands(b, edges((0, 1)), None, np.array([0, 8, 1, 0], dtype=np.uint32))
    assert of.tolist() == [0, 0, 1, 2]
    assert rows(rec) == [(0, 2, 1, 0, 0, 1), (2, 1, 0, 0, 0, 1), (3, 1, 0, 0, 0, 0)]
    assert rec["max_speed2"].tolist() == [36.0, 0.0, 3.0] and rec["max_angular_speed2"].tolist() == [4.0, 0.0, 0.0]


def test_a_nan_velocity_shows_as_a_nan_and_negative_zero_as_zero():
    b = bodies(3, velocity={0: (1.0e200, 0.0, 0.0), 1: (np.nan, 0.0, 0.0)}, angular={2: (-0.0, 0.0, 0.0)})
    of, rec = im.islands(b, edges((0, 1)), None, no_masks(3))
    assert of.tolist() == [0, 0, 1]
    assert np.isnan(rec["max_speed2"][0]) and rec["max_speed2"][1] == 0.0      # (1e200 squared is +inf: the NaN still wins)
    assert rec["max_angular_speed2"].view(np.uint64).tolist() == [0, 0]


def test_masks_from_the_contact_list():
    masks = im.masks_from_contacts(4, np.array([[1, 0], [1, 3], [3, 7]], dtype=np.uint32))
    assert masks.tolist() == [0, 9, 0, 128]


# ---- the layout of xpbd_island ------------------------------------------------------------------------------------------
C_TYPES = {"uint32_t": ("<u4", 4), "double": ("<f8", 8)}


def header_island_fields():
    text = open(os.path.join(ROOT, "include", "xpbd.h")).read()
    body = re.search(r"typedef struct xpbd_island \{(.*?)\} xpbd_island;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields, at = [], 0
    for ctype, name in re.findall(r"(uint32_t|double)\s+(\w+);", body):
        kind, size = C_TYPES[ctype]
        at = (at + size - 1) // size * size          # natural alignment
        fields.append((name, kind, at))
        at += size
    return fields, (at + 7) // 8 * 8


def test_struct_size_and_offsets_match_the_header():
    fields, size = header_island_fields()
    assert size == 40 and len(fields) == 8
    for dtype in (capi.ISLAND_DTYPE, im.ISLAND_DTYPE):
        assert dtype.itemsize == size
        assert [(name, dtype.fields[name][0].str, dtype.fields[name][1]) for name in dtype.names] == fields
    text = open(os.path.join(ROOT, "include", "xpbd.h")).read()
    for name, value in (("XPBD_ISLAND_NONE", capi.ISLAND_NONE), ("XPBD_ISLANDS_NO_JOINTS", capi.ISLANDS_NO_JOINTS),
                        ("XPBD_ISLANDS_NO_CONTACTS", capi.ISLANDS_NO_CONTACTS)):
        assert int(re.search(r"#define %s\s+(\w+?)u\b" % name, text).group(1), 0) == value
    assert (im.ISLAND_NONE, im.NO_JOINTS, im.NO_CONTACTS) == (capi.ISLAND_NONE, capi.ISLANDS_NO_JOINTS, capi.ISLANDS_NO_CONTACTS)
