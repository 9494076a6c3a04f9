"""Shared by the joint-state and drive-target tests and their torch child process (joint_state_device_child.py): the scenes,
the retarget lists, and the runs that the host variant (in the test process) and the device variant (in the child) both make,
so that their results can be compared bit for bit."""
import math

import numpy as np

import joint_drive_model as jd
from constraint_solver_amd import capi

DT = 1.0 / 60.0
SUBSTEPS = 4
FRAMES = 3                    # "a few frames of stepping" before the states are read
SMALL_WORLD = 16384           # xpbd_contacts.hip: up to this many bodies the pair solve runs eight lanes per body
INF = float("inf")
N_RECIPES = 14
STATE_WORLDS = (65, 257)      # joints: a wave boundary and a block boundary of k_joint_states (the 1-joint worlds: every recipe)
NO_LIMITS = np.zeros(0, dtype=capi.JOINT_LIMIT_DTYPE)


def _unit(v):
    return v / np.linalg.norm(v)


def mechanisms(n_joints, seed, extra_bodies=0):
    """n_joints separate two-body mechanisms on a 6 m x 8 m grid, 3 m up, no gravity: tilted, drifting and spinning, their anchors
    assembled at the start; every third base is static.  Joint k follows recipe (k + seed) % N_RECIPES, so 14 joints in a row show
    every joint kind, every limit kind and every drive kind, alone and together; limits and drives are listed in a shuffled
    order.  extra_bodies: free bodies appended behind the mechanisms, jointed to nobody.
    Returns bodies, shape ids, joints, limits, drives."""
    rng = np.random.default_rng(7000 + seed)
    n = 2 * n_joints + extra_bodies
    bodies, sid = capi.scene_generate(capi.SCENE_BOXES, 1, n)
    bodies[:, 10:22] = 0.0
    joints = np.zeros(n_joints, dtype=capi.JOINT_DTYPE)
    lims, drvs = [], []
    for i in range(n):
        k, end = divmod(i, 2)
        axis, angle = _unit(rng.normal(size=3)), rng.uniform(-0.3, 0.3)
        bodies[i, 31:34] = [6.0 * (k % 16) + 2.0 * end, 8.0 * (k // 16), 3.0]
        bodies[i, 34:38] = np.concatenate([[math.cos(angle / 2)], axis * math.sin(angle / 2)])
        bodies[i, 22:25] = rng.normal(scale=0.3, size=3)
        bodies[i, 25:28] = rng.normal(scale=2.0, size=3)
    for k in range(n_joints):
        if k % 3 == 0:
            bodies[2 * k, 0:10] = 0.0
        j = joints[k]
        j["body_a"], j["body_b"] = 2 * k, 2 * k + 1
        j["anchor_a"], j["anchor_b"] = [1.5, 0.5, 0.5], [-0.5, 0.5, 0.5]
        axis = _unit(rng.normal(size=3))
        ref, ref2 = _unit(np.cross(axis, rng.normal(size=3))), _unit(np.cross(axis, rng.normal(size=3)))
        j["axis_a"] = j["axis_b"] = axis
        lo, sl = rng.uniform(-0.2, 0.0), rng.uniform(-0.05, 0.0)
        hinge_limit = dict(joint=k, kind=capi.LIMIT_HINGE, ref_a=ref2, ref_b=ref2, lower=lo, upper=lo + rng.uniform(0.0, 0.2))
        slide_limit = dict(joint=k, kind=capi.LIMIT_SLIDE, lower=sl, upper=sl + rng.uniform(0.0, 0.05))
        soft = rng.uniform(0.0, 0.01) if rng.uniform() < 0.5 else 0.0
        weak = rng.uniform(0.5, 5.0) if rng.uniform() < 0.5 else INF

        def drive(kind, target, refs=True):
            return dict(joint=k, kind=kind, target=target, compliance=soft, max_force=weak, ref_a=ref if refs else 0.0, ref_b=ref if refs else 0.0)

        recipe = (k + seed) % N_RECIPES
        j["kind"] = capi.JOINT_HINGE if recipe in (0, 1, 2, 3, 13) else (capi.JOINT_SLIDER if recipe in (4, 5, 6, 7) else capi.JOINT_DISTANCE)
        if recipe == 0:
            lims.append(hinge_limit)
        elif recipe == 1:
            drvs.append(drive(capi.DRIVE_ANGLE, rng.uniform(-0.3, 0.3)))
        elif recipe == 2:                                            # the drive's references are not the limit's
            drvs.append(drive(capi.DRIVE_ANGULAR_VELOCITY, rng.uniform(-5.0, 5.0)))
            lims.append(hinge_limit)
        elif recipe == 4:
            lims.append(slide_limit)
            drvs.append(drive(capi.DRIVE_POSITION, rng.uniform(-0.2, 0.2), refs=False))
        elif recipe == 5:
            drvs.append(drive(capi.DRIVE_VELOCITY, rng.uniform(-2.0, 2.0), refs=False))
            lims.append(hinge_limit)
        elif recipe == 6:                                            # two drives on one joint, and a SLIDE limit
            drvs.append(drive(capi.DRIVE_VELOCITY, rng.uniform(-2.0, 2.0), refs=False))
            drvs.append(drive(capi.DRIVE_ANGLE, rng.uniform(-0.3, 0.3)))
            lims.append(slide_limit)
        elif recipe == 9:
            j["distance"] = 0.3
        elif recipe in (10, 11, 12):
            if recipe != 11:
                lims.append(dict(joint=k, kind=capi.LIMIT_SWING, lower=0.0, upper=rng.uniform(0.05, 0.4)))
            if recipe != 10:
                lims.append(dict(joint=k, kind=capi.LIMIT_TWIST, ref_a=ref, ref_b=ref, lower=lo, upper=lo + rng.uniform(0.0, 0.2)))
        elif recipe == 13:                                           # the encoder idiom: a limit that never binds
            lims.append(dict(joint=k, kind=capi.LIMIT_HINGE, ref_a=ref, ref_b=ref, lower=-math.pi, upper=math.pi))
        if recipe in (8, 9):                                         # a ball joint needs no axes
            j["axis_a"] = j["axis_b"] = 0.0
    lims = [lims[i] for i in rng.permutation(len(lims))]
    drvs = [drvs[i] for i in rng.permutation(len(drvs))]
    return bodies, sid, joints, jd.records(capi.JOINT_LIMIT_DTYPE, *lims), jd.records(capi.JOINT_DRIVE_DTYPE, *drvs)


def with_fillers(bodies, sid, n_total):
    """The scene with resting boxes on a far grid appended up to n_total bodies (they touch nothing and never move)."""
    n_fill = n_total - len(bodies)
    fill, fill_sid = capi.scene_generate(capi.SCENE_BOXES, 2, n_fill)
    fill[:, 10:28] = 0.0
    fill[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    side = int(math.ceil(math.sqrt(n_fill)))
    fill[:, 31] = 300.0 + 3.0 * (np.arange(n_fill) % side)
    fill[:, 32] = 300.0 + 3.0 * (np.arange(n_fill) // side)
    fill[:, 33] = 3.0
    return np.concatenate([bodies, fill]), np.concatenate([sid, fill_sid])


def new_world(bodies, sid, joints, lims, drvs):
    w = capi.World(mode=capi.MODE_CONTACTS)
    w.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES))
    w.upload(bodies, sid)
    w.set_joints(joints)
    w.set_joint_limits(lims)
    w.set_joint_drives(drvs)
    return w


def stepped_world(n_joints, seed):
    """(world after FRAMES frames, the scene) of mechanisms(n_joints, seed)."""
    scene = mechanisms(n_joints, seed)
    w = new_world(*scene)
    for _ in range(FRAMES):
        w.step(DT, SUBSTEPS)
    return w, scene


# ---- drive targets ----------------------------------------------------------------------------------------------------
N_DRIVEN = 28                 # joints of the retarget scene: every recipe twice
DRIVEN_SEED = 1
RETARGET_AT, RETARGET_THEN = 2, 3


def driven_scene(big, extra_bodies=0):
    bodies, sid, joints, lims, drvs = mechanisms(N_DRIVEN, DRIVEN_SEED, extra_bodies)
    n_mech = len(bodies)
    if big:
        bodies, sid = with_fillers(bodies, sid, SMALL_WORLD + 64)
    return bodies, sid, joints, lims, drvs, n_mech


def new_targets(drvs, seed=0):
    """A fresh, valid target for every drive, far from the present one."""
    rng = np.random.default_rng(9000 + seed)
    span = {capi.DRIVE_ANGLE: 0.3, capi.DRIVE_ANGULAR_VELOCITY: 5.0, capi.DRIVE_POSITION: 0.2, capi.DRIVE_VELOCITY: 2.0}
    return np.array([rng.uniform(-span[int(k)], span[int(k)]) for k in drvs["kind"]])


def some_drives(drvs):
    """An ascending subset of the drives (every other one, the last included) and their new targets."""
    idx = np.unique(np.concatenate([np.arange(0, len(drvs), 2), [len(drvs) - 1]])).astype(np.uint32)
    return idx, new_targets(drvs)[idx]


def invalid_list(drvs):
    """(drives, targets, valid) of a retarget list with every kind of bad entry among good ones: out of range, not above its
    predecessor, NaN, infinite, an ANGLE target of 4.0.  valid[k]: what the device variant applies (an entry is compared with
    its predecessor in the list whether or not that one counted)."""
    n = len(drvs)
    angle = [int(d) for d in np.flatnonzero(drvs["kind"] == capi.DRIVE_ANGLE)]
    other = [int(d) for d in np.flatnonzero(drvs["kind"] != capi.DRIVE_ANGLE)]
    assert len(angle) >= 2 and len(other) >= 6
    drives, targets = list(range(n)), list(new_targets(drvs, 1))      # every drive, ascending, with a good target ...
    targets[other[0]] = float("nan")                                  # ... then the defects
    targets[other[2]] = INF
    targets[other[4]] = -INF
    targets[angle[0]] = 4.0
    at = other[3] if other[3] + 1 < n else other[1]                   # a descent: two neighbours change places
    drives[at], drives[at + 1] = drives[at + 1], drives[at]
    drives += [n - 1, n, 0xFFFFFFFF]                                  # a repeat, and two indices out of range
    targets += [0.125, 0.5, 0.5]
    drives, targets = np.array(drives, dtype=np.uint32), np.array(targets)
    valid = np.zeros(len(drives), dtype=bool)
    seen = set()
    for k, (d, t) in enumerate(zip(drives, targets)):
        why = ("range" if d >= n else "order" if k and drives[k - 1] >= d else "finite" if not math.isfinite(t) else
               "angle" if drvs["kind"][d] == capi.DRIVE_ANGLE and not -math.pi <= t <= math.pi else "")
        seen.add(why)
        valid[k] = why == ""
    assert seen == {"", "range", "order", "finite", "angle"} and valid.sum() >= 6
    return drives, targets, valid


def retarget_run(retarget, big, drives, targets, extra=None):
    """The retarget scene: RETARGET_AT frames, retarget(w, drives, targets), optionally extra(w, scene), RETARGET_THEN frames.
    Returns the mechanisms' rows."""
    scene = driven_scene(big)
    with new_world(*scene[:5]) as w:
        for _ in range(RETARGET_AT):
            w.step(DT, SUBSTEPS)
        retarget(w, drives, targets)
        for _ in range(RETARGET_THEN):
            w.step(DT, SUBSTEPS)
        return w.download()[:scene[5]]


def host_retarget(w, drives, targets):
    w.set_drive_targets(drives, targets)


def table_retarget(drvs):
    """The same change through xpbd_world_set_joint_drives: the whole table with the new targets."""
    def apply(w, drives, targets):
        table = drvs.copy()
        table["target"][np.arange(len(drvs)) if drives is None else drives] = targets
        w.set_joint_drives(table)
    return apply


# ---- sleeping ---------------------------------------------------------------------------------------------------------
SLEEP_CFG = (0.5, 2.0, 5)     # linear_speed, angular_speed, frames_to_sleep
SLEEP_FRAMES = 40
SLEEP_SUBSTEPS = 10


def resting_mechanisms():
    """Three separate mechanisms at rest on the ground, 20 m apart: two boxes side by side, hinged about z, with a soft ANGLE drive
    at its target.  Bodies 0-1 and 2-3 are free; body 4, the base of the third, is fixed.  Drive k belongs to mechanism k."""
    bodies, _ = capi.scene_generate(capi.SCENE_BOXES, 3, 6)
    bodies[:, 22:28] = 0.0
    bodies[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    for i in range(6):
        bodies[i, 31:34] = [20.0 * (i // 2) + 1.5 * (i % 2), 0.0, 0.0]
    bodies[4, 0:10] = 0.0
    joints = np.zeros(3, dtype=capi.JOINT_DTYPE)
    joints["body_a"], joints["body_b"] = [0, 2, 4], [1, 3, 5]
    joints["anchor_a"], joints["anchor_b"] = [1.25, 0.5, 0.5], [-0.25, 0.5, 0.5]
    joints["axis_a"] = joints["axis_b"] = [0.0, 0.0, 1.0]
    joints["kind"] = capi.JOINT_HINGE
    x = [1.0, 0.0, 0.0]
    drvs = jd.records(capi.JOINT_DRIVE_DTYPE, *[dict(joint=k, kind=capi.DRIVE_ANGLE, ref_a=x, ref_b=x, target=0.0, compliance=0.01, max_force=INF)
                                                for k in range(3)])
    return bodies, np.zeros(6, dtype=np.uint32), joints, drvs


def sleeping_world():
    """resting_mechanisms() with sleeping on, stepped until everybody who can sleep does.  Returns (world, drives)."""
    bodies, sid, joints, drvs = resting_mechanisms()
    w = capi.World(mode=capi.MODE_CONTACTS)
    w.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES))
    w.upload(bodies, sid)
    w.set_joints(joints)
    w.set_joint_drives(drvs)
    w.set_contact_report(True)
    w.set_sleeping(*SLEEP_CFG)
    for _ in range(SLEEP_FRAMES):
        w.step(DT, SLEEP_SUBSTEPS)
    return w, drvs


def wake_sequence(w, drvs, retarget):
    """asleep[] after: settling; a retarget of the drive on the fixed base; a retarget of mechanism 0's drive; the same change once
    more through xpbd_world_set_joint_drives.  One step follows each."""
    out = [w.sleep_state()[0].copy()]
    for drive in (2, 0):
        retarget(w, np.array([drive], dtype=np.uint32), np.array([0.3]))
        w.step(DT, SLEEP_SUBSTEPS)
        out.append(w.sleep_state()[0].copy())
    table = drvs.copy()
    table["target"][[0, 2]] = 0.3
    w.set_joint_drives(table)
    w.step(DT, SLEEP_SUBSTEPS)
    out.append(w.sleep_state()[0].copy())
    return np.array(out)


# ---- the closed loop --------------------------------------------------------------------------------------------------
LOOP_GAIN, LOOP_GOAL, LOOP_FRAMES = 10.0, 0.5, 60


def loop_scene():
    """The wheel of tests/joint_drive_model.py: a free body hinged about z on a static base, with an ANGULAR_VELOCITY drive."""
    rows, joints, limits, drives, _, _, _ = jd.scene("wheel")
    drives = drives.copy()
    drives["target"] = 0.0
    return rows, joints.astype(capi.JOINT_DTYPE), limits.astype(capi.JOINT_LIMIT_DTYPE), drives.astype(capi.JOINT_DRIVE_DTYPE)
