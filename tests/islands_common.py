"""Shared by test_gpu_islands.py and its torch child process (islands_device_child.py): the joint graphs, the crafted scene, the
small box drop, and the comparison of a world's islands with the independent model (islands_model.py)."""
import numpy as np

import islands_model as im
from constraint_solver_amd import capi

DT = 1.0 / 60.0
BOXES = capi.SCENE_BOXES
SLAB = 4.0                   # edge of the crafted scene's fixed slab (shape 1), metres


def distance_joints(a, b, distance=1.0):
    """Distance joints between the centres of the unit boxes a[k] and b[k], in the given orientation."""
    a, b = np.asarray(a, dtype=np.uint32).reshape(-1), np.asarray(b, dtype=np.uint32).reshape(-1)
    j = np.zeros(a.size, dtype=capi.JOINT_DTYPE)
    j["body_a"], j["body_b"] = a, b
    j["anchor_a"], j["anchor_b"], j["distance"] = [0.5, 0.5, 0.5], [0.5, 0.5, 0.5], distance
    return j


def spread_bodies(n, seed=11, fixed=()):
    """n boxes of the seeded scene, 10 m apart on a line (nothing touches, nothing is stepped), the listed ones fixed."""
    bodies, sid = capi.scene_generate(BOXES, seed, n)
    bodies[:, 31], bodies[:, 32], bodies[:, 33] = 10.0 * np.arange(n), 0.0, 5.0
    for i in fixed:
        bodies[i, 0:10] = 0.0
    return bodies, sid


def graph_world(bodies, sid, joints):
    w = capi.World(mode=capi.MODE_CONTACTS)
    w.set_polytopes(capi.scene_polytopes(BOXES))
    w.upload(bodies, sid)
    if len(joints):
        w.set_joints(joints)
    return w


def crafted_scene():
    """16 bodies: two three-box stacks on the ground (0-2, 3-5); a fixed slab (6) with two boxes resting apart on it (7, 8); a
    fixed post (9) with a five-link chain hanging from it (10-14); one box in free fall (15).  Returns (bodies, shape ids,
    joints); shape 0 is the unit box, shape 1 the slab."""
    bodies, _ = capi.scene_generate(BOXES, 3, 16)
    bodies[:, 22:28] = 0.0
    bodies[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    gap = 0.002
    at = np.zeros((16, 3))
    for k in range(3):
        at[k] = [0.0, 0.0, k * (1.0 + gap)]
        at[3 + k] = [5.0, 0.0, k * (1.0 + gap)]
    at[6] = [10.0, 0.0, 0.0]
    at[7] = [10.5, 1.5, SLAB + gap]
    at[8] = [12.5, 1.5, SLAB + gap]
    at[9] = [20.0, 0.0, 10.0]
    for k in range(5):
        at[10 + k] = [20.0, 0.0, 10.0 - 1.5 * (k + 1)]
    at[15] = [30.0, 0.0, 50.0]
    bodies[:, 31:34] = at
    sid = np.zeros(16, dtype=np.uint32)
    sid[6] = 1
    bodies[6, 28:31] = SLAB / 2
    for i in (6, 9):
        bodies[i, 0:10] = 0.0
    joints = distance_joints(np.arange(9, 14), np.arange(10, 15), 1.5)
    return bodies, sid, joints


def crafted_world(narrowphase=capi.NARROWPHASE_SAT, report=True):
    bodies, sid, joints = crafted_scene()
    w = capi.World(mode=capi.MODE_CONTACTS)
    w.set_polytopes([capi.polytope(capi.SHAPE_CUBE), capi.polytope(capi.SHAPE_CUBE, SLAB)])
    w.set_narrowphase(narrowphase)
    w.upload(bodies, sid)
    w.set_joints(joints)
    if report:
        w.set_contact_report(True)
    return w, joints


def drop_scene(n=512, seed=1, fixed=()):
    """The benchmark's box pile at small size (capi.scene_pile, 4 layers at 1.8 m), lowered so that it lands within a few frames,
    with chains of five boxes along x joined by distance joints at the pitch (bench.py's chain_joints without its hinges)."""
    pitch, layers = 1.8, 4
    bodies, sid = capi.scene_pile(capi.SCENE_BOXES_DROP, seed, n, pitch, layers, lift=0.45)
    for i in fixed:
        bodies[i, 0:10] = 0.0
        bodies[i, 22:28] = 0.0
    grid_w = capi.default_grid_width((n + layers - 1) // layers)
    k = np.arange((n // 5) * 4)
    a = (k // 4) * 5 + (k % 4)
    per_layer = (n + layers - 1) // layers
    keep = (a + 1 < n) & ((a % per_layer) // grid_w == ((a + 1) % per_layer) // grid_w) & (a // per_layer == (a + 1) // per_layer)
    a = a[keep][::3]                                     # some boxes carry joints, most do not
    return bodies, sid, distance_joints(a, a + 1, pitch)


def drop_world(narrowphase=capi.NARROWPHASE_SAT, report=True, n=512, fixed=()):
    bodies, sid, joints = drop_scene(n, fixed=fixed)
    w = capi.World(mode=capi.MODE_CONTACTS)
    w.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES_DROP))
    w.set_narrowphase(narrowphase)
    w.upload(bodies, sid)
    w.set_joints(joints)
    if report:
        w.set_contact_report(True)
    return w, joints


def model_of(w, joints, flags):
    """The model's answer for the world as a host can download it."""
    bodies = w.download()
    pairs = None if flags & capi.ISLANDS_NO_CONTACTS else w.pair_contacts(points=False)[0]
    masks = im.masks_from_contacts(w.n, w.contacts())
    return im.islands(bodies, pairs, joints, masks, flags)


def assert_equals_model(w, joints, flags):
    """The library's island_of and records equal the model's, bit for bit; returns them."""
    got_of, got = w.islands(flags)
    want_of, want = model_of(w, joints, flags)
    assert im.same_bytes(got_of, want_of), (flags, np.flatnonzero(got_of != want_of)[:8])
    assert got.dtype == want.dtype and len(got) == len(want), (flags, len(got), len(want))
    for name in got.dtype.names:
        assert im.same_bytes(got[name], want[name]), (flags, name, got[name][:8], want[name][:8])
    assert im.same_bytes(got, want)
    return got_of, got
