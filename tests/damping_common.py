"""Shared by the damping tests (test_damping_model.py, test_gpu_damping.py): the scenes, their damping tables and the expected
frames by the model (damping_model.py), computed once per process.

Shapes: 16 to 32 unit boxes, 8 substeps, 3 or 4 frames.  Every scene fits one wave, so awake, FIXED and capped bodies share it."""
import functools
import math

import numpy as np

import damping_model as dm
import kinematic_common as kc
import restitution_model as rm
from constraint_solver_amd import capi

DT = kc.DT
PAD = kc.PAD
SUBSTEPS = 8
FRAMES = 4
H = DT / SUBSTEPS
INF = math.inf
NO_JOINTS = kc.NO_JOINTS
N_PILE = 18
PILE_FIXED = 4                 # the centre box of the base layer
N_CHAIN = 8                    # a fixed root, six links, and the body on the ball joint
RESTITUTION = 0.5


def polys():
    return kc.polys()


def new_world(bodies, sid, joints=None, narrowphase=capi.NARROWPHASE_SAT):
    w = kc.new_world(bodies, sid, joints)
    w.set_narrowphase(narrowphase)
    return w


# ---- the pile: a base layer at rest, a second layer dropped onto it ---------------------------------------------------------
def pile_scene():
    """18 unit boxes: nine resting on the plane on a 3 x 3 grid (the centre one FIXED), nine above them, shifted, coming down at
    2 to 3 m/s with some spin and drift, so the first frame already has contacts and the layer tips and piles."""
    rng = np.random.default_rng(5100)
    at = [[1.1 * (k % 3), 1.1 * (k // 3), 0.0] for k in range(9)]
    at += [[1.1 * (k % 3) + 0.35, 1.1 * (k // 3) + 0.25, 1.05] for k in range(9)]
    bodies, sid = kc.boxes(N_PILE, at, fixed=[PILE_FIXED])
    bodies[9:, 22:24] = rng.uniform(-0.5, 0.5, (9, 2))
    bodies[9:, 24] = rng.uniform(-3.0, -2.0, 9)
    bodies[9:, 25:28] = rng.uniform(-2.0, 2.0, (9, 3))
    return bodies, sid


def pile_rows(n=N_PILE):
    """Mixed drag on everybody (some rows zero), caps on every third body: low enough that they fire for the falling layer in some
    substeps and not in others, never for the resting one."""
    rng = np.random.default_rng(5200)
    rows = dm.rows(n, linear=rng.choice([0.0, 0.5, 2.0, 10.0], n), angular=rng.choice([0.0, 0.5, 2.0, 10.0], n))
    rows["max_linear_speed"][::3] = 1.5
    rows["max_angular_speed"][::3] = 1.0
    return rows


# ---- the chain: six hinged links from a fixed root, and a body on a ball joint at its end -----------------------------------
def chain_scene(origin=(0.0, 10.0, 6.0)):
    """Body 0 FIXED; bodies 1-6 links 1.2 m apart along x, hinged about y to their predecessor; body 7 on a ball joint behind the
    last link.  Released horizontally with a little drift and spin.  Joints 0-5 the hinges in chain order, joint 6 the ball."""
    rng = np.random.default_rng(5300)
    at = [[origin[0] + 1.2 * k, origin[1], origin[2]] for k in range(N_CHAIN)]
    bodies, sid = kc.boxes(N_CHAIN, at, fixed=[0])
    bodies[1:, 22:25] = rng.uniform(-0.3, 0.3, (N_CHAIN - 1, 3))
    bodies[1:, 25:28] = rng.uniform(-1.0, 1.0, (N_CHAIN - 1, 3))
    joints = np.zeros(N_CHAIN - 1, dtype=capi.JOINT_DTYPE)
    for k in range(N_CHAIN - 1):
        j = joints[k]
        j["body_a"], j["body_b"] = k, k + 1
        j["anchor_a"], j["anchor_b"] = [1.1, 0.5, 0.5], [-0.1, 0.5, 0.5]
        if k < 6:
            j["kind"] = capi.JOINT_HINGE
            j["axis_a"] = j["axis_b"] = [0.0, 1.0, 0.0]
    return bodies, sid, joints


def chain_dampers(first_joint=0):
    """Linear and angular dampers on alternating hinges, one hinge with both, one with none, and both on the ball joint: the
    links between them have one or two entries, so the two ends of a joint divide by different counts."""
    f = first_joint
    return dm.dampers((f + 0, 30.0, 0.0), (f + 1, 0.0, 40.0), (f + 2, 25.0, 600.0), (f + 4, 500.0, 0.0), (f + 5, 0.0, 20.0), (f + 6, 15.0, 35.0))


def chain_on_pile_scene():
    """The pile with the chain 0.25 m above its top layer: the links come down on it within the first frames."""
    pile, pile_sid = pile_scene()
    chain, chain_sid, joints = chain_scene(origin=(-1.3, 1.35, 2.3))
    joints = joints.copy()
    joints["body_a"] += N_PILE
    joints["body_b"] += N_PILE
    return np.concatenate([pile, chain]), np.concatenate([pile_sid, chain_sid]), joints


def chain_on_pile_rows():
    rows = dm.rows(N_PILE + N_CHAIN)
    rows[:N_PILE] = pile_rows()
    rows["linear"][N_PILE + 2], rows["max_angular_speed"][N_PILE + 5] = 1.0, 0.8
    return rows


# ---- the scenes of "GPU == model" and what the model expects of them ---------------------------------------------------------
# name -> (bodies, sid, joints, body rows or None, joint dampers or None, restitution or None)
def scene(name):
    if name == "pile":
        bodies, sid = pile_scene()
        return bodies, sid, NO_JOINTS, pile_rows(), None, None
    if name == "pile_bouncing":
        bodies, sid = pile_scene()
        return bodies, sid, NO_JOINTS, pile_rows(), None, RESTITUTION
    if name == "chain":
        bodies, sid, joints = chain_scene()
        return bodies, sid, joints, None, chain_dampers(), None
    if name == "chain_on_pile":
        bodies, sid, joints = chain_on_pile_scene()
        return bodies, sid, joints, chain_on_pile_rows(), chain_dampers(), None
    raise KeyError(name)


SCENES = ("pile", "pile_bouncing", "chain", "chain_on_pile")


@functools.lru_cache(maxsize=None)
def expected(name, narrowphase=0, damped=True):
    """The rows after each of FRAMES frames by the model (damped=False: the same scene without stage 7)."""
    bodies, sid, joints, rows, dampers, e = scene(name)
    if not damped:
        rows = dampers = None
    if e is not None:
        model = rm.Model(bodies, sid, polys(), e=[e] * len(bodies), ground_e=e)
        return [dm.restitution_substeps(model, DT, SUBSTEPS, rows).copy() for _ in range(FRAMES)]
    return dm.expected_frames(bodies, sid, polys(), joints, DT, SUBSTEPS, PAD, FRAMES, rows, dampers, narrowphase)


def run_world(name, narrowphase=capi.NARROWPHASE_SAT):
    """The rows after each of FRAMES frames by the library."""
    bodies, sid, joints, rows, dampers, e = scene(name)
    out = []
    with new_world(bodies, sid, joints, narrowphase) as w:
        if e is not None:
            w.set_restitution([e] * len(bodies), e)
        if rows is not None:
            w.set_damping(rows)
        if dampers is not None:
            w.set_joint_damping(dampers)
        for _ in range(FRAMES):
            w.step(DT, SUBSTEPS)
            out.append(w.download())
    return out


# ---- caps: a light box squeezed between two heavy ones -----------------------------------------------------------------------
CAP_LINEAR, CAP_ANGULAR = 3.0, 5.0
SQUEEZE_FRAMES = 4


def squeeze_scene():
    """Two heavy boxes on the plane 1.7 m apart and a box a hundred times lighter between them, 0.3 m up, overlapping one by
    0.1 m and the other by 0.2 m: the contacts resolve the overlap within one substep and the light box leaves at 6.6 m/s and
    11.7 rad/s (the model's figures)."""
    bodies, sid = kc.boxes(3, [[0.0, 0.0, 0.0], [0.9, 0.1, 0.3], [1.7, 0.0, 0.0]])
    bodies[1, 0:10] *= 100.0                                          # inverse mass and inverse inertia
    bodies[1, 10:22] /= 100.0                                         # its weight with it
    return bodies, sid


def speeds(rows):
    return np.linalg.norm(rows[:, 22:25], axis=1), np.linalg.norm(rows[:, 25:28], axis=1)


# ---- a damper damps: a box on a hinge from a fixed body, released at 60 degrees ----------------------------------------------
PENDULUM_ARM = 1.5             # hinge to the box's centre
PENDULUM_SECONDS = 6


def pendulum_scene(angle=math.pi / 3.0):
    """Body 0 FIXED with the hinge (axis y) at its centre; body 1 hangs from it by an anchor 1.5 m above its own centre, turned by
    `angle` about the hinge.  An XPBD_LIMIT_HINGE of [-pi, pi] never binds and gives the hinge its encoder."""
    bodies, sid = kc.boxes(2, [[0.0, 0.0, 6.0], [0.0, 0.0, 0.0]], fixed=[0])
    pivot = np.array([0.5, 0.5, 6.5])
    anchor_b = np.array([0.5, 0.5, 0.5 + PENDULUM_ARM])
    c, s = math.cos(angle), math.sin(angle)
    rot = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])      # about y
    com = bodies[1, 28:31]
    origin = pivot - rot @ anchor_b                                   # Rigid::frame() origin: pivot = origin + rot * anchor_b
    bodies[1, 31:34] = origin - com + rot @ com
    bodies[1, 34:38] = [math.cos(angle / 2.0), 0.0, math.sin(angle / 2.0), 0.0]
    joints = np.zeros(1, dtype=capi.JOINT_DTYPE)
    joints[0]["body_a"], joints[0]["body_b"], joints[0]["kind"] = 0, 1, capi.JOINT_HINGE
    joints[0]["anchor_a"], joints[0]["anchor_b"] = [0.5, 0.5, 0.5], anchor_b
    joints[0]["axis_a"] = joints[0]["axis_b"] = [0.0, 1.0, 0.0]
    limits = np.zeros(1, dtype=capi.JOINT_LIMIT_DTYPE)
    limits[0]["joint"], limits[0]["kind"] = 0, capi.LIMIT_HINGE
    limits[0]["ref_a"] = limits[0]["ref_b"] = [1.0, 0.0, 0.0]
    limits[0]["lower"], limits[0]["upper"] = -math.pi, math.pi
    return bodies, sid, joints, limits


def swing_peaks(rates):
    """The largest |angle_rate| of every swing: the runs between sign changes of the rate."""
    peaks, cur, sign = [], 0.0, 0
    for r in rates:
        s = int(r > 0.0) - int(r < 0.0)
        if s and sign and s != sign:
            peaks.append(cur)
            cur = 0.0
        if s:
            sign = s
        cur = max(cur, abs(r))
    return peaks


# ---- sleeping: the 3-stack that cycles for ever ------------------------------------------------------------------------------
# The angular threshold is below the stack's jitter ("Sleeping": it cycles at 0.018 m/s and 0.111 rad/s), so without
# drag it never rests.  Drag does not remove the jitter, which the position pass makes anew in every substep: it moves the stack
# to another cycle, of 0.009 to 0.012 m/s and 0.051 or 0.11 rad/s depending on the coefficient (measured on the model, DESIGN.md
# 8, "Damping"), so the thresholds sit between the two: twice the damped cycle < threshold, angular < the undamped one.
# SLEEP_DRAG and SLEEP_MODEL_FRAME are determined on the CPU model by tests/test_damping_model.py, which asserts them.
SLEEP_CFG = (0.03, 0.105, 10)  # linear_speed, angular_speed, frames_to_sleep
SLEEP_SUBSTEPS = 20
SLEEP_CANDIDATES = (1.0, 2.0, 5.0, 10.0, 20.0)
SLEEP_MODEL_BUDGET = 80        # frames the model may take to bring the stack under half the thresholds for good
SLEEP_DRAG = 2.0               # 1/s, on every body: the smallest of SLEEP_CANDIDATES that does it ...
SLEEP_MODEL_FRAME = 40         # ... and the frame from which on the model's stack stays under half the thresholds
SLEEP_FRAMES = math.ceil(1.25 * (SLEEP_MODEL_FRAME + SLEEP_CFG[2]))    # the budget: that, frames_to_sleep, and a quarter more
