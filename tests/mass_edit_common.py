"""Shared by the mass-edit tests (test_gpu_mass_edit.py, test_gpu_mass_edit_sleeping.py) and their torch child process
(mass_edit_device_child.py): the scenes, the rows, and the runs that the host variant (in the test process) and the device variant
(in the child) both make, so that results compare bit for bit.  Every run takes `edit(w, indices, rows, flags)`."""
import numpy as np

import mass_edit_model as mm
from constraint_solver_amd import capi

DT = 1.0 / 60.0
SUBSTEPS = 20
GAP = 0.002
IDENT = (1.0, 0.0, 0.0, 0.0)
MASS = mm.MASS_COLUMNS
DYN = list(range(22, 28)) + list(range(31, 38))          # the 13 dynamic doubles of an xpbd_rigid row
OTHERS = [c for c in range(38) if c not in MASS]         # the 25 doubles a mass edit without KEEP_FRAME leaves alone


def host_edit(w, indices, rows, flags=mm.INVERSE):
    w.set_mass_properties(indices, rows, flags)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def boxes(positions, fixed=()):
    """Identical unit boxes at rest, upright, at `positions` (the min corner): one mass row for all of them, the listed ones fixed."""
    n = len(positions)
    bodies, _ = capi.scene_generate(capi.SCENE_BOXES, 3, n)
    bodies[:] = bodies[0]                                 # (mass properties and the scene's gravity, the same bits for all)
    bodies[:, 22:28] = 0.0
    bodies[:, 34:38] = IDENT
    bodies[:, 31:34] = positions
    for i in fixed:
        bodies[i, 0:10] = 0.0
    return bodies, np.zeros(n, dtype=np.uint32)


def new_world(bodies, sid, mode=capi.MODE_CONTACTS, narrowphase=capi.NARROWPHASE_SAT, trace=False):
    w = capi.World(mode=mode, trace_contacts=trace)
    w.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES))
    if mode == capi.MODE_CONTACTS:
        w.set_narrowphase(narrowphase)
    w.upload(bodies, sid)
    return w


# ---- 1. round trip: 7 bodies with distinct mass rows ----------------------------------------------------------------------------
N_TRIP = 7
TRIP_LISTS = {"unordered": [5, 0, 6, 2, 1, 4, 3], "subset": [6, 1, 3], "all": None}


def trip_scene():
    rng = np.random.default_rng(6100)
    bodies, sid = boxes([[3.0 * i, 0.0, 2.0] for i in range(N_TRIP)])
    bodies[:, 0] *= rng.uniform(0.5, 2.0, N_TRIP)
    bodies[:, 1:10] *= rng.uniform(0.5, 2.0, (N_TRIP, 1))
    bodies[:, 28:31] += rng.uniform(-0.1, 0.1, (N_TRIP, 3))
    bodies[:, 22:28] = rng.normal(size=(N_TRIP, 6))
    return bodies, sid


def trip_rows(n, seed=6200):
    """n valid INVERSE rows, all different (one of them fixed, one with inverse_mass 0 and inertia)."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 13))
    rows[:, 0] = rng.uniform(0.1, 3.0, n)
    a = rng.normal(size=(n, 3, 3))
    rows[:, 1:10] = (a @ a.transpose(0, 2, 1) + np.eye(3)).reshape(n, 9)
    rows[:, 10:13] = rng.uniform(-0.3, 0.3, (n, 3))
    rows[0, 0:10] = 0.0
    if n > 1:
        rows[1, 0] = 0.0
    return rows


def trip_run(edit, which):
    """The round-trip scene after one frame, edited: (download before, get before, download after, get after, rows)."""
    bodies, sid = trip_scene()
    idx = TRIP_LISTS[which]
    rows = trip_rows(N_TRIP if idx is None else len(idx))
    with new_world(bodies, sid) as w:
        w.step(DT, SUBSTEPS)
        before, got_before = w.download(), w.get_mass_properties(idx)
        edit(w, idx, rows, mm.INVERSE)
        return before, got_before, w.download(), w.get_mass_properties(idx), rows


# ---- 2. the property: a block of identical boxes on the shared-mass path ------------------------------------------------------
BLOCK_SIDE = 4
PRE_FRAMES, POST_FRAMES = 2, 3
HEAVY, FROZEN, SHIFTED = 37, 5, 42
HINGE, SLIDER = (60, 61), (62, 63)          # neighbours along x in the top layer


def block_scene(side=BLOCK_SIDE):
    """side^3 identical unit boxes, 2 mm apart, 1 cm above the plane; body i + side * j + side^2 * k."""
    pitch = 1.0 + GAP
    at = [[pitch * i, pitch * j, 0.01 + pitch * k] for k in range(side) for j in range(side) for i in range(side)]
    return boxes(at)


def block_settings(w):
    """One hinge, one slider with a velocity drive, filters, friction 0.5, restitution 0.3, the contact report."""
    joints = np.zeros(2, dtype=capi.JOINT_DTYPE)
    joints["body_a"], joints["body_b"] = [HINGE[0], SLIDER[0]], [HINGE[1], SLIDER[1]]
    joints["anchor_a"], joints["anchor_b"] = [1.0 + GAP / 2, 0.5, 0.5], [-GAP / 2, 0.5, 0.5]
    joints["axis_a"], joints["axis_b"] = [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0]]
    joints["kind"] = [capi.JOINT_HINGE, capi.JOINT_SLIDER]
    drives = np.zeros(1, dtype=capi.JOINT_DRIVE_DTYPE)
    drives["joint"], drives["kind"], drives["target"], drives["max_force"] = 1, capi.DRIVE_VELOCITY, 0.2, np.inf
    filters = np.zeros(w.n, dtype=capi.COLLISION_FILTER_DTYPE)
    filters["group"], filters["mask"] = 1 << (np.arange(w.n) % 2), 3
    filters["mask"][::7] = 1
    w.set_joints(joints)
    w.set_joint_drives(drives)
    w.set_collision_filters(filters, capi.FILTER_JOINTED)
    w.set_materials(np.full(w.n, 0.5), 0.5)
    w.set_restitution(np.full(w.n, 0.3), 0.3, 0.0)
    w.set_contact_report(True)
    return joints


def block_edits(rows):
    """[(indices, rows, flags)] of the three-body edit from the 13 doubles the bodies have: HEAVY ten times heavier, FROZEN
    fixed, SHIFTED with its centre of mass moved by (0.1, 0, 0) and the geometry kept."""
    heavy, frozen, shifted = rows[HEAVY].copy(), rows[FROZEN].copy(), rows[SHIFTED].copy()
    heavy[0:10] /= 10.0
    frozen[0:10] = 0.0
    shifted[10] += 0.1
    return [([HEAVY, FROZEN], np.stack([heavy, frozen]), mm.INVERSE), ([SHIFTED], shifted[None, :], mm.INVERSE | mm.KEEP_FRAME)]


def all_edit(rows):
    """Every body gets the same new row, twice as heavy: a fresh upload shares the per-shape table again, the edited world does not."""
    row = rows[0].copy()
    row[0:10] /= 2.0
    return [(None, np.tile(row, (len(rows), 1)), mm.INVERSE)]


class Snapshot:
    """What a host can see after a frame of XPBD_MODE_CONTACTS with the report on."""

    def __init__(self, w, report=True):
        self.bodies, self.contacts, self.masks = w.download(), np.asarray(w.contacts()).copy(), w.contact_masks(SUBSTEPS)
        if report:
            self.pairs, self.points = w.pair_contacts()
            self.events, self.counts = w.contact_events(), w.contact_report_counts()

    def assert_equal(self, other, where):
        for name in self.__dict__:
            a, b = getattr(self, name), getattr(other, name)
            assert (a == b if isinstance(a, tuple) else same(a, b)), (where, name)


def block_run(edit, edits_of, narrowphase=capi.NARROWPHASE_SAT, side=BLOCK_SIDE):
    """PRE_FRAMES frames, the edit, POST_FRAMES frames: (the download right after the edit, the snapshot of every later frame)."""
    bodies, sid = block_scene(side)
    with new_world(bodies, sid, narrowphase=narrowphase, trace=True) as w:
        block_settings(w)
        for _ in range(PRE_FRAMES):
            w.step(DT, SUBSTEPS)
        for idx, rows, flags in edits_of(w.get_mass_properties()):
            edit(w, idx, rows, flags)
        edited = w.download()
        frames = []
        for _ in range(POST_FRAMES):
            w.step(DT, SUBSTEPS)
            frames.append(Snapshot(w))
        return edited, frames


def block_fresh(edited, narrowphase=capi.NARROWPHASE_SAT):
    """A fresh world uploaded with the post-edit download and the same settings, stepped POST_FRAMES frames."""
    with new_world(edited, np.zeros(len(edited), dtype=np.uint32), narrowphase=narrowphase, trace=True) as w:
        block_settings(w)
        frames = []
        for _ in range(POST_FRAMES):
            w.step(DT, SUBSTEPS)
            frames.append(Snapshot(w))
        return frames


# ---- 3. DIRECT: random positive-definite rows ----------------------------------------------------------------------------------
N_DIRECT, N_DIRECT_BODIES = 32, 40
SINGULAR_AT = 11


def direct_scene():
    return boxes([[3.0 * (i % 8), 3.0 * (i // 8), 2.0] for i in range(N_DIRECT_BODIES)])


def direct_rows(singular=False):
    """(indices, rows): N_DIRECT distinct bodies in a shuffled order, mass, a positive-definite tensor over six decades, a centre
    of mass; with `singular` entry SINGULAR_AT has two equal columns."""
    rng = np.random.default_rng(6300)
    idx = rng.permutation(N_DIRECT_BODIES)[:N_DIRECT].astype(np.uint32)
    rows = np.zeros((N_DIRECT, 13))
    rows[:, 0] = 10.0 ** rng.uniform(-2, 3, N_DIRECT)
    a = rng.normal(size=(N_DIRECT, 3, 3)) * 10.0 ** rng.uniform(-3, 3, (N_DIRECT, 1, 1))
    rows[:, 1:10] = (a @ a.transpose(0, 2, 1) + 1e-3 * np.eye(3) * np.trace(a @ a.transpose(0, 2, 1), axis1=1, axis2=2)[:, None, None]).reshape(-1, 9)
    rows[:, 10:13] = rng.uniform(-0.3, 0.3, (N_DIRECT, 3))
    if singular:
        rows[SINGULAR_AT, 4:7] = rows[SINGULAR_AT, 1:4]
    return idx, rows


def direct_run(edit, singular=False):
    """(download before, download after) of the DIRECT edit."""
    bodies, sid = direct_scene()
    idx, rows = direct_rows(singular)
    with new_world(bodies, sid) as w:
        before = w.download()
        edit(w, idx, rows, mm.DIRECT)
        return before, w.download()


# ---- 4. KEEP_FRAME: random poses far from the origin ----------------------------------------------------------------------------
N_KEEP = 16


def keep_scene():
    rng = np.random.default_rng(6400)
    bodies, sid = boxes(rng.uniform(-1e3, 1e3, (N_KEEP, 3)))
    q = rng.normal(size=(N_KEEP, 4))
    bodies[:, 34:38] = q / np.linalg.norm(q, axis=1)[:, None]
    bodies[:, 22:25] = rng.normal(size=(N_KEEP, 3))
    bodies[:, 25:28] = rng.normal(scale=3.0, size=(N_KEEP, 3))
    rows = bodies[:, MASS].copy()
    rows[:, 10:13] = rng.uniform(-0.5, 0.5, (N_KEEP, 3))
    rows[3, 10:13] = bodies[3, 28:31]                     # one centre of mass does not move: d == 0
    return bodies, sid, rows


def keep_run(edit):
    """(download before, frames before, download after, frames after, rows) of the KEEP_FRAME edit of every body."""
    bodies, sid, rows = keep_scene()
    with new_world(bodies, sid) as w:
        before, frames_before = w.download(), w.frames()
        edit(w, None, rows, mm.INVERSE | mm.KEEP_FRAME)
        return before, frames_before, w.download(), w.frames(), rows


# ---- 7. sleeping: two 3-stacks ---------------------------------------------------------------------------------------------------
SLEEP_CFG = (0.1, 0.5, 4)      # linear_speed, angular_speed, frames_to_sleep
SETTLE_FRAMES = 40
STACK_A, STACK_B = (0, 1, 2), (3, 4, 5)
ANCHOR = 6                     # a fixed box hovering far from both stacks
MIDDLE = STACK_A[1]


def stacks_scene():
    at = [[x, 0.0, k * (1.0 + GAP)] for x in (0.0, 20.0) for k in range(3)] + [[40.0, 0.0, 5.0]]
    return boxes(at, fixed=[ANCHOR])


def stacks_world():
    bodies, sid = stacks_scene()
    w = new_world(bodies, sid)
    w.set_contact_report(True)
    w.set_sleeping(*SLEEP_CFG)
    return w
