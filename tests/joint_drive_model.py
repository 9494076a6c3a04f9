"""Independent model of XPBD_MODE_CONTACTS for jointed bodies that touch nothing, with sliders, SLIDE limits and joint
drives: one substep is integrate, the Jacobi joint pass with every term, and derive.

Written from include/xpbd.h ("Joints", "Angular joint LIMITS", "SLIDERS and joint DRIVES") in plain f64 numpy, not from
the kernels and without calling oracle/.  The vector helpers and the body of tests/joint_limit_model.py are reused; the
joint pass is this file's own.  Its operation order is its own, so it agrees with the device to rounding, not bit for bit.

A body is a row of 38 doubles (xpbd_rigid); joints, limits and drives are numpy records of capi.JOINT_DTYPE /
JOINT_LIMIT_DTYPE / JOINT_DRIVE_DTYPE (any record type with those field names will do: no device library is needed).
"""
import math

import numpy as np

from joint_limit_model import Body, _norm, _normalized_q, _pure, limit_angle
from xprec_model import conj, cross, dot, matvec, qmul, qrot

JOINT_DISTANCE, JOINT_HINGE, JOINT_SLIDER = 0, 1, 2
LIMIT_HINGE, LIMIT_SWING, LIMIT_TWIST, LIMIT_SLIDE = 0, 1, 2, 3
DRIVE_ANGLE, DRIVE_ANGULAR_VELOCITY, DRIVE_POSITION, DRIVE_VELOCITY = 0, 1, 2, 3

JOINT_DTYPE = np.dtype([("body_a", "<u4"), ("body_b", "<u4"), ("anchor_a", "<f8", (3,)), ("anchor_b", "<f8", (3,)),
                        ("distance", "<f8"), ("axis_a", "<f8", (3,)), ("axis_b", "<f8", (3,)), ("kind", "<u4"), ("reserved", "<u4")])
LIMIT_DTYPE = np.dtype([("joint", "<u4"), ("kind", "<u4"), ("ref_a", "<f8", (3,)), ("ref_b", "<f8", (3,)), ("lower", "<f8"), ("upper", "<f8")])
DRIVE_DTYPE = np.dtype([("joint", "<u4"), ("kind", "<u4"), ("ref_a", "<f8", (3,)), ("ref_b", "<f8", (3,)),
                        ("target", "<f8"), ("compliance", "<f8"), ("max_force", "<f8")])


def wrap(x):
    return x - 2 * math.pi if x > math.pi else (x + 2 * math.pi if x < -math.pi else x)


class Pose:
    """A body at another pose (the start of the substep): what Body.point needs."""

    def __init__(self, body, pos, rot):
        self.pos, self.rot, self.com = pos, rot, body.com

    point = Body.point


def _linear_w(body, p, n):
    """Constraint::inverse_resitance: m^-1 + (I^-1 r) . r with r the arm x n taken into the body's space."""
    r = qrot(conj(body.rot), cross(p - (body.pos + body.com), n))
    return body.im + dot(matvec(body.M, r), r)


def _linear(ia, ib, a, b, p_a, p_b, n, lam):
    """+lam n on a at p_a, -lam n on b at p_b (Rigid::apply_impulse: the spin is (I^-1 arm) x impulse, world-space arm)."""
    return [(ia, lam * n * a.im, cross(matvec(a.M, p_a - (a.pos + a.com)), lam * n)),
            (ib, -lam * n * b.im, cross(matvec(b.M, p_b - (b.pos + b.com)), -lam * n))]


def _angular(ia, ib, a, b, n, lam):
    return [(ia, np.zeros(3), matvec(a.M, lam * n)), (ib, np.zeros(3), matvec(b.M, -lam * n))]


def slide_offset(joint, a, b):
    """(s, d, a_w, p_a, p_b) of a joint for two bodies (or Poses): the offset of b's anchor along a's axis."""
    p_a, p_b = a.point(joint["anchor_a"]), b.point(joint["anchor_b"])
    a_w = qrot(a.rot, np.asarray(joint["axis_a"], dtype=np.float64))
    d = p_b - p_a
    return dot(d, a_w), d, a_w, p_a, p_b


def hinge_angle(joint, ref_a, ref_b, q_a, q_b):
    return limit_angle(LIMIT_HINGE, q_a, q_b, joint["axis_a"], joint["axis_b"], ref_a, ref_b)[0]


def _joint_entries(bodies, past, joint, limits, drives, h):
    """Every Jacobi entry of one joint: a list of (body, dpos, spin)."""
    c = 1e-6 / (h * h)
    ia, ib = int(joint["body_a"]), int(joint["body_b"])
    a, b = bodies[ia], bodies[ib]
    kind = int(joint["kind"])
    out = []
    s, d, a_w, p_a, p_b = slide_offset(joint, a, b)
    dist = _norm(d)
    if kind != JOINT_SLIDER and dist != 0.0:                           # the positional term
        n = d / dist
        lam = (dist - float(joint["distance"])) / (_linear_w(a, p_a, n) + _linear_w(b, p_b, n) + c)
        out += _linear(ia, ib, a, b, p_a, p_b, n, lam)
    if kind != JOINT_DISTANCE:                                         # the hinge's angular term: HINGE and SLIDER
        delta = cross(a_w, qrot(b.rot, np.asarray(joint["axis_b"], dtype=np.float64)))
        mag = _norm(delta)
        if mag != 0.0:
            n = delta / mag
            out += _angular(ia, ib, a, b, n, mag / (a.angular_w(n) + b.angular_w(n) + c))
    for lim in limits:                                                 # the angular limits, the caller's order
        if int(lim["kind"]) == LIMIT_SLIDE:
            continue
        got = limit_angle(int(lim["kind"]), a.rot, b.rot, joint["axis_a"], joint["axis_b"], lim["ref_a"], lim["ref_b"])
        if got is None:
            continue
        phi, n = got
        err = phi - min(max(phi, float(lim["lower"])), float(lim["upper"]))
        if err != 0.0:
            out += _angular(ia, ib, a, b, n, err / (a.angular_w(n) + b.angular_w(n) + c))
    # ---- the extra entries -------------------------------------------------------------------------------------------
    if kind == JOINT_SLIDER:                                           # 1. perpendicular term
        r = d - a_w * s
        length = _norm(r)
        if length != 0.0:
            n = r / length
            out += _linear(ia, ib, a, b, p_a, p_b, n, length / (_linear_w(a, p_a, n) + _linear_w(b, p_b, n) + c))
    for lim in limits:                                                 # 2. the SLIDE limit
        if int(lim["kind"]) != LIMIT_SLIDE:
            continue
        e = s - min(max(s, float(lim["lower"])), float(lim["upper"]))
        if e != 0.0:
            out += _linear(ia, ib, a, b, p_a, p_b, a_w, e / (_linear_w(a, p_a, a_w) + _linear_w(b, p_b, a_w) + c))
    pa, pb = Pose(a, *past[ia]), Pose(b, *past[ib])
    for drv in drives:                                                 # 3. the drives, the caller's order
        k, target = int(drv["kind"]), float(drv["target"])
        if k in (DRIVE_ANGLE, DRIVE_ANGULAR_VELOCITY):
            phi = hinge_angle(joint, drv["ref_a"], drv["ref_b"], a.rot, b.rot)
            if k == DRIVE_ANGLE:
                e = wrap(phi - target)
            else:
                e = wrap(phi - hinge_angle(joint, drv["ref_a"], drv["ref_b"], pa.rot, pb.rot)) - target * h
            w = a.angular_w(a_w) + b.angular_w(a_w)
        elif k in (DRIVE_POSITION, DRIVE_VELOCITY):
            e = s - target if k == DRIVE_POSITION else (s - slide_offset(joint, pa, pb)[0]) - target * h
            w = _linear_w(a, p_a, a_w) + _linear_w(b, p_b, a_w)
        else:
            raise ValueError("unknown drive kind %r" % k)
        if e == 0.0:
            continue
        lam = e / (w + (1e-6 + float(drv["compliance"])) / (h * h))
        cap = float(drv["max_force"]) * (h * h)
        lam = min(max(lam, -cap), cap)
        out += _angular(ia, ib, a, b, a_w, lam) if k in (DRIVE_ANGLE, DRIVE_ANGULAR_VELOCITY) else _linear(ia, ib, a, b, p_a, p_b, a_w, lam)
    return out


def substep(rows, joints, limits, drives, h):
    """One substep of (n, 38) f64 body rows; returns the new rows."""
    rows = np.array(rows, dtype=np.float64).reshape(-1, 38)
    bodies = [Body(r) for r in rows]
    past = [(b.pos.copy(), b.rot.copy()) for b in bodies]
    for b in bodies:                                                 # Rigid::integrate
        b.vel = b.vel + (b.ef + qrot(b.rot, b.fi)) * h * b.im
        b.pos = b.pos + b.vel * h
        b.ang = b.ang + matvec(b.M, b.et + qrot(b.rot, b.ti)) * h
        b.rot = _normalized_q(b.rot + qmul(_pure(b.ang) * (h / 2), b.rot))
    # the Jacobi pass: every entry is evaluated on the post-integrate poses, each body averages its own entries
    dpos = [np.zeros(3) for _ in bodies]
    drot = [np.zeros(4) for _ in bodies]
    count = [0] * len(bodies)
    lim_of = [[] for _ in range(len(joints))]
    drv_of = [[] for _ in range(len(joints))]
    for lim in limits:
        lim_of[int(lim["joint"])].append(lim)
    for drv in drives:
        drv_of[int(drv["joint"])].append(drv)
    for k, joint in enumerate(joints):
        for i, dp, spin in _joint_entries(bodies, past, joint, lim_of[k], drv_of[k], h):
            dpos[i] = dpos[i] + dp
            drot[i] = drot[i] + qmul(_pure(spin) * 0.5, bodies[i].rot)
            count[i] += 1
    for i, b in enumerate(bodies):
        if count[i]:
            b.pos = b.pos + dpos[i] / count[i]
            b.rot = _normalized_q(b.rot + drot[i] / count[i])
    for (pp, pr), b, row in zip(past, bodies, rows):                 # Rigid::derive
        b.vel = (b.pos - pp) / h
        dq = qmul(b.rot, conj(pr))
        if dq[0] < 0:
            dq = -dq
        b.ang = dq[1:] * 2 / h
        row[22:25], row[25:28], row[31:34], row[34:38] = b.vel, b.ang, b.pos, b.rot
    return rows


def step(rows, joints, limits, drives, dt, substeps):
    """xpbd_world_step(dt, substeps) of the model."""
    h = dt / substeps
    for _ in range(substeps):
        rows = substep(rows, joints, limits, drives, h)
    return rows


# ---- the known-answer scenes (tests/test_joint_drive_model.py on the model, tests/test_gpu_joint_drives.py on the device) ----
X, Y, Z = [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]
G = 9.81


def two_rows(pos_b=(0.0, 0.0, 20.0)):
    """A static base (body 0) and a free unit-mass body with the inertia of a unit cube (body 1), both with their centre of
    mass at their position and the joint's anchors there too: every impulse of the joint acts at b's centre.  High above the
    ground and, where a device runs it, 6 m apart: nothing touches."""
    rows = np.zeros((2, 38))
    rows[:, 34] = 1.0
    rows[0, 31:34] = [pos_b[0] - 6.0, pos_b[1], pos_b[2]]
    rows[1, 31:34] = pos_b
    rows[1, 0] = 1.0
    rows[1, [1, 5, 9]] = 6.0
    return rows


def one_joint(kind, axis, joint_dtype=JOINT_DTYPE):
    j = np.zeros(1, dtype=joint_dtype)
    j["body_a"], j["body_b"], j["kind"] = 0, 1, kind
    j["anchor_a"] = [6.0, 0.0, 0.0]
    j["axis_a"] = j["axis_b"] = axis
    return j


def records(dtype, *rows):
    out = np.zeros(len(rows), dtype=dtype)
    for k, r in enumerate(rows):
        for name, value in r.items():
            out[k][name] = value
    return out


def perpendicular_to(axis):
    axis = np.asarray(axis, dtype=np.float64)
    ref = np.cross(axis, [0.0, 1.0, 0.0] if abs(axis[1]) < 0.9 else [1.0, 0.0, 0.0])
    return ref / np.linalg.norm(ref)


def angle_and_offset(rows, joint, ref=None):
    """(phi about the axis from ref to ref, s along the axis, |d - a_w s|) of body 0 -> body 1 through `joint`."""
    a, b = Body(rows[int(joint["body_a"])]), Body(rows[int(joint["body_b"])])
    ref = perpendicular_to(joint["axis_a"]) if ref is None else ref
    s, d, a_w, _, _ = slide_offset(joint, a, b)
    return hinge_angle(joint, ref, ref, a.rot, b.rot), s, _norm(d - a_w * s)


DT = 1.0 / 60.0
WHEEL_SPEED = 3.0                      # rad/s
SPRING_TARGET, SPRING_TORQUE, SPRING_COMPLIANCE = 0.2, 20.0, 0.002
TILT = 0.5                             # rad below the horizontal
LIFT_SPEED, LIFT_WEAK, LIFT_STRONG = 1.0, 5.0, 20.0
SLIDE_STOP = 0.3                       # m
INF = float("inf")
NO_LIMITS, NO_DRIVES = np.zeros(0, dtype=LIMIT_DTYPE), np.zeros(0, dtype=DRIVE_DTYPE)


def scene(name):
    """(rows, joints, limits, drives, steps, substeps, dt) of a known-answer scene: `steps` calls of step(dt, substeps)."""
    rows = two_rows()
    ref = perpendicular_to(Z)
    if name == "wheel":                # a free wheel on a static base, driven at WHEEL_SPEED
        joints = one_joint(JOINT_HINGE, Z)
        drives = records(DRIVE_DTYPE, dict(joint=0, kind=DRIVE_ANGULAR_VELOCITY, ref_a=ref, ref_b=ref, target=WHEEL_SPEED, max_force=INF))
        return rows, joints, NO_LIMITS, drives, 3, 20, DT
    if name == "spring":               # an angular spring (ANGLE drive with compliance) loaded by a constant torque
        joints = one_joint(JOINT_HINGE, Z)
        rows[1, 16:19] = [0.0, 0.0, SPRING_TORQUE]
        drives = records(DRIVE_DTYPE, dict(joint=0, kind=DRIVE_ANGLE, ref_a=ref, ref_b=ref, target=SPRING_TARGET,
                                           compliance=SPRING_COMPLIANCE, max_force=INF))
        return rows, joints, NO_LIMITS, drives, 100, 2, DT
    if name in ("incline", "incline_stop", "incline_free"):   # a slider whose axis points TILT below the horizontal, under gravity
        joints = one_joint(JOINT_SLIDER, [math.cos(TILT), 0.0, -math.sin(TILT)])
        rows[1, 10:13] = [0.0, 0.0, -G]
        if name == "incline":
            return rows, joints, NO_LIMITS, NO_DRIVES, 30, 20, DT
        # ... with a stop SLIDE_STOP down the axis, looked at after every substep (incline_free: the control without the stop)
        limits = records(LIMIT_DTYPE, dict(joint=0, kind=LIMIT_SLIDE, lower=-SLIDE_STOP, upper=SLIDE_STOP)) if name == "incline_stop" else NO_LIMITS
        return rows, joints, limits, NO_DRIVES, 600, 1, DT / 20
    if name in ("lift_weak", "lift_strong"):  # a vertical slider lifting 1 kg at LIFT_SPEED with a motor of limited force
        joints = one_joint(JOINT_SLIDER, Z)
        rows[1, 10:13] = [0.0, 0.0, -G]
        force = LIFT_WEAK if name == "lift_weak" else LIFT_STRONG
        drives = records(DRIVE_DTYPE, dict(joint=0, kind=DRIVE_VELOCITY, target=LIFT_SPEED, max_force=force))
        return rows, joints, NO_LIMITS, drives, 30, 20, DT
    if name in ("prismatic", "cylindrical"):  # a slider along x, sliding and spinning, looked at after every substep; the hinge
        joints = one_joint(JOINT_SLIDER, X)   # limit 0/0 (prismatic) takes the spin away, the control (cylindrical) keeps it
        rows[1, 22:25] = [1.0, 0.0, 0.0]
        rows[1, 25:28] = [5.0, 0.0, 0.0]
        ref = perpendicular_to(X)
        limits = records(LIMIT_DTYPE, dict(joint=0, kind=LIMIT_HINGE, ref_a=ref, ref_b=ref)) if name == "prismatic" else NO_LIMITS
        return rows, joints, limits, NO_DRIVES, 240, 1, DT / 20
    raise ValueError(name)


def run_scene(name, stepper=None):
    """The rows after every step call of a scene.  stepper(rows, joints, limits, drives, steps, substeps, dt) -> list of
    rows; the default is the model."""
    rows, joints, limits, drives, steps, substeps, dt = scene(name)
    if stepper is not None:
        return stepper(rows, joints, limits, drives, steps, substeps, dt)
    out = []
    for _ in range(steps):
        rows = step(rows, joints, limits, drives, dt, substeps)
        out.append(rows)
    return out


FIGURES = {"wheel": "wheel", "spring": "spring", "incline": "incline", "incline_perpendicular": "incline", "incline_stop": "incline_stop",
           "incline_free": "incline_free", "lift_weak": "lift_weak", "lift_strong": "lift_strong", "prismatic": "prismatic",
           "cylindrical": "cylindrical"}   # figure -> the scene it is read from


def measure(name, path):
    """The figure of a known-answer scene and the known answer: (value, answer).  path: run_scene of FIGURES[name]."""
    rows, joints, limits, drives, steps, substeps, dt = scene(FIGURES[name])
    joint, last, t = joints[0], path[-1], steps * dt
    axis = np.asarray(joint["axis_a"], dtype=np.float64)
    if name == "wheel":                # the wheel turns at the drive's speed: its angle advances by speed * dt in the last frame
        return (angle_and_offset(last, joint)[0] - angle_and_offset(path[-2], joint)[0]) / dt, WHEEL_SPEED
    if name == "spring":               # torque = (phi - target) / compliance
        return angle_and_offset(last, joint)[0], SPRING_TARGET + SPRING_TORQUE * SPRING_COMPLIANCE
    if name == "incline":              # it accelerates at g sin(tilt) along the axis
        return float(np.dot(last[1, 22:25], axis)), G * math.sin(TILT) * t
    if name == "incline_perpendicular":   # ... and stays on the axis
        return max(angle_and_offset(r, joint)[2] for r in path), 0.0
    if name in ("incline_stop", "incline_free"):   # the farthest it gets: the stop (the control: the free slide's 1/2 a t^2)
        return max(angle_and_offset(r, joint)[1] for r in path), SLIDE_STOP if name == "incline_stop" else 0.5 * G * math.sin(TILT) * t * t
    if name == "lift_weak":            # the motor stalls: the load falls against max_force
        return last[1, 24], -(G - LIFT_WEAK) * t
    if name == "lift_strong":          # the motor lifts at its speed
        return last[1, 24], LIFT_SPEED
    if name in ("prismatic", "cylindrical"):   # the largest angle about the axis: none (the control: it turns on)
        return max(abs(angle_and_offset(r, joint)[0]) for r in path), 0.0
    raise ValueError(name)
