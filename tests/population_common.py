"""Shared by test_gpu_population.py and its torch child process (population_device_child.py): the settings of the 130-body
scenes of body_edit_common.py, their re-index in numpy -- independent of the library -- and what a run is compared by."""
import numpy as np

from body_edit_common import DT, N, SUBSTEPS, scene
from constraint_solver_amd import capi
from halo_common import chain_joints

NO_HIT = capi.NO_HIT
X, Z = [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]
HINGES, SLIDERS = (1, 20), (7, 30)          # joints 2-5 and 40-43; 14-17 and 60-63 of chain_joints(N): body 2k to 2k + 3
REMOVED = np.array([5, 63, 64, 129, 33, 64], dtype=np.uint32)   # ends of joints 1 and 30 among them, wave boundaries, one twice


def settings_for(n=N, seed=8):
    """The settings of test_gpu_body_edits.py's settings() -- joints with a hinge limit, filters with FILTER_JOINTED, friction,
    restitution, the contact report -- plus sliders with SLIDE limits and drives, limits and drives listed out of joint order."""
    rng = np.random.default_rng(seed)
    joints = chain_joints(capi, n)
    joints["axis_a"], joints["axis_b"] = Z, Z
    for j in HINGES:
        joints["kind"][j] = capi.JOINT_HINGE
    for j in SLIDERS:
        joints["kind"][j], joints["distance"][j] = capi.JOINT_SLIDER, 0.0
    extra = joints[[3, 3, 9]].copy()                                     # a pair joined twice more, and one given with body_a > body_b
    extra["body_a"][2], extra["body_b"][2] = joints["body_b"][9], joints["body_a"][9]
    extra["distance"] = [1.25, 1.75, 2.0]
    joints = np.concatenate([joints, extra])
    lims = np.zeros(5, dtype=capi.JOINT_LIMIT_DTYPE)
    lims["joint"] = [SLIDERS[1], HINGES[0], SLIDERS[0], HINGES[1], SLIDERS[0]]
    lims["kind"] = [capi.LIMIT_SLIDE, capi.LIMIT_HINGE, capi.LIMIT_SLIDE, capi.LIMIT_HINGE, capi.LIMIT_HINGE]
    lims["lower"], lims["upper"] = [-0.3, -0.2, -0.1, -0.4, -0.5], [0.4, 0.3, 0.2, 0.1, 0.6]
    lims["ref_a"], lims["ref_b"] = X, X
    drives = np.zeros(4, dtype=capi.JOINT_DRIVE_DTYPE)
    drives["joint"] = [SLIDERS[0], HINGES[0], SLIDERS[1], HINGES[1]]
    drives["kind"] = [capi.DRIVE_POSITION, capi.DRIVE_ANGULAR_VELOCITY, capi.DRIVE_VELOCITY, capi.DRIVE_ANGLE]
    drives["target"], drives["compliance"], drives["max_force"] = [0.1, 2.0, -0.5, 0.2], [0.0, 0.001, 0.0, 0.002], [np.inf, 50.0, 20.0, np.inf]
    drives["ref_a"], drives["ref_b"] = X, X
    filters = np.zeros(n, dtype=capi.COLLISION_FILTER_DTYPE)
    filters["group"], filters["mask"] = 1 << rng.integers(0, 2, n), 3
    filters["mask"][::7] = 1
    return dict(joints=joints, lims=lims, drives=drives, filters=filters, mu=rng.uniform(0.1, 0.9, n), e=rng.uniform(0.2, 0.8, n))


def apply_settings(w, s, report=True):
    w.set_joints(s["joints"])
    w.set_joint_limits(s["lims"])
    w.set_joint_drives(s["drives"])
    w.set_collision_filters(s["filters"], capi.FILTER_JOINTED)
    w.set_materials(s["mu"], 0.6)
    w.set_restitution(s["e"], 0.5, 0.1)
    if report:
        w.set_contact_report(True)


def expected_map(n, removed):
    """old_to_new of removing `removed` from n bodies, by the header's definition."""
    keep = np.ones(n, dtype=bool)
    keep[np.asarray(removed, dtype=np.int64)] = False
    return np.where(keep, np.cumsum(keep) - 1, NO_HIT).astype(np.uint32), keep


def reindex_joints(s, old_to_new):
    """(joints, lims, drives, joint_old_to_new) after the bodies were re-indexed: numpy only."""
    j = s["joints"]
    alive = (old_to_new[j["body_a"]] != NO_HIT) & (old_to_new[j["body_b"]] != NO_HIT)
    jmap = np.where(alive, np.cumsum(alive) - 1, NO_HIT).astype(np.uint32)
    joints = j[alive].copy()
    joints["body_a"], joints["body_b"] = old_to_new[joints["body_a"]], old_to_new[joints["body_b"]]
    lims = s["lims"][jmap[s["lims"]["joint"]] != NO_HIT].copy()
    lims["joint"] = jmap[lims["joint"]]
    drives = s["drives"][jmap[s["drives"]["joint"]] != NO_HIT].copy()
    drives["joint"] = jmap[drives["joint"]]
    return joints, lims, drives, jmap


def reindex_settings(s, old_to_new, n_add):
    """The settings a fresh world needs after `old_to_new` and n_add appended bodies with the defaults."""
    keep = old_to_new != NO_HIT
    joints, lims, drives, _ = reindex_joints(s, old_to_new)
    default = np.zeros(n_add, dtype=capi.COLLISION_FILTER_DTYPE)
    default["group"] = default["mask"] = 0xFFFFFFFF
    return dict(joints=joints, lims=lims, drives=drives, filters=np.concatenate([s["filters"][keep], default]),
                mu=np.concatenate([s["mu"][keep], np.full(n_add, np.inf)]), e=np.concatenate([s["e"][keep], np.zeros(n_add)]))


def newcomers(kind, count, seed=99):
    """`count` bodies of another seed's scene, spread out above the pile."""
    bodies, sid = scene(kind, seed)
    rows = np.arange(3, 3 + count)
    bodies, sid = bodies[rows].copy(), sid[rows].copy()
    bodies[:, 31] = 0.7 + 1.3 * np.arange(count)
    bodies[:, 32] = 2.5
    bodies[:, 33] = 7.5 + 0.25 * np.arange(count)
    return bodies, sid


def trigger_volume():
    """Three unit boxes (shape 0 of the box scene) inside the pile: "who is inside this trigger?"."""
    return capi.overlap_queries([[2.5, 2.5, 1.0], [1.5, 3.0, 2.0], [3.5, 1.5, 1.5]], [1.0, 0.0, 0.0, 0.0], 0)


def run(w, frames, contacts_mode):
    """Everything two worlds are compared by after `frames` frames: bodies, ground contacts and, in the contact pipeline, the
    contact report's pairs, points and events of every frame and the neighbour lists of the final state."""
    out = []
    for _ in range(frames):
        w.step(DT, SUBSTEPS)
        if contacts_mode:
            pairs, points = w.pair_contacts()
            out += [pairs, points, w.contact_events()]
    out += [w.download(), w.contacts()]
    if contacts_mode:
        out += list(w.neighbours(DT))
    return out


def same_runs(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes() for x, y in zip(a, b))
