"""Independent model of KINEMATIC bodies (include/xpbd.h, "KINEMATIC bodies") in plain Python floats, written from the header:
the velocity overwrite before the integrate stage of every substep, and the expected frames of a world that has a kinematic table.

Python's float arithmetic is IEEE double, one rounding per operation and no contraction, which is what the header asks for;
math.atan2 and math.tan are the platform's libm (correctly rounded or within an ulp, which the device's are not: the GPU tests
hold rotations to a measured tolerance and translations to the bit).

Expected frames come from the committed oracle (oracle_binding.contacts_step_joints) run ONE SUBSTEP at a time, with this model's
velocities written into the kinematic bodies before each call.  tests/test_kinematic_model.py shows first that the oracle run
per substep equals the oracle run per frame bit for bit on every scene used that way, with the platform held static."""
import math

import numpy as np

import oracle_binding as ob

POSE, VELOCITY = 0, 1
VEL, ANG, POS, ROT = slice(22, 25), slice(25, 28), slice(31, 34), slice(34, 38)
TABLE_DTYPE = np.dtype([("body", np.uint32), ("mode", np.uint32), ("linear", np.float64, 3), ("angular", np.float64, 4)])


def table(*entries):
    """entries: (body, mode, linear[3], angular[3 or 4])."""
    t = np.zeros(len(entries), dtype=TABLE_DTYPE)
    for k, (body, mode, linear, angular) in enumerate(entries):
        t[k]["body"], t[k]["mode"], t[k]["linear"] = body, mode, linear
        t[k]["angular"][:len(angular)] = angular
    return t


def qmul(a, b):
    """Hamilton product, {s, x, y, z}, each component summed left to right."""
    return (a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
            a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
            a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
            a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1])


def pose_velocities(p, q, p_t, q_t, h, r):
    """(velocity, angular_velocity) of a POSE entry with r substeps of h left, from the current position p and rotation q."""
    rh = float(r) * h
    vel = tuple((p_t[c] - p[c]) / rh for c in range(3))
    dq = qmul(q_t, (q[0], -q[1], -q[2], -q[3]))
    if dq[0] < 0.0:
        dq = tuple(-x for x in dq)
    v = dq[1:]
    m = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
    if m == 0.0:
        return vel, (0.0, 0.0, 0.0)
    half = math.atan2(m, dq[0])
    k = (2.0 / h) * math.tan(half / float(r)) / m
    return vel, tuple(x * k for x in v)


def velocities(entry, row, h, r):
    """The two velocities entry `entry` (a TABLE_DTYPE record) gives the body whose xpbd_rigid row is `row`."""
    lin, ang = [float(x) for x in entry["linear"]], [float(x) for x in entry["angular"]]
    if int(entry["mode"]) == POSE:
        return pose_velocities([float(x) for x in row[POS]], [float(x) for x in row[ROT]], lin, ang, h, r)
    return tuple(lin), tuple(ang[:3])


def overwrite(rows, tbl, h, r):
    """rows with the overwrite of a substep that has r substeps of h left applied (a copy); and who is MOVING by it."""
    out = np.array(rows, dtype=np.float64).reshape(-1, 38).copy()
    moving = np.zeros(len(out), dtype=bool)
    for e in tbl:
        i = int(e["body"])
        vel, ang = velocities(e, out[i], h, r)
        out[i, VEL], out[i, ANG] = vel, ang
        moving[i] = any(x != 0.0 for x in vel + ang)
    return out, moving


def integrate_pose(p, q, vel, ang, h):
    """What the integrate stage does to the pose of a body without forces: position + h * velocity, and the rotation update
    normalized(q + ((h / 2) * {0, w}) * q) of the stepper, operation for operation."""
    p1 = tuple(p[c] + h * vel[c] for c in range(3))
    k = h * 0.5
    dq = qmul((k * 0.0, k * ang[0], k * ang[1], k * ang[2]), q)
    s = tuple(q[c] + dq[c] for c in range(4))
    n = 1.0 / math.sqrt(s[0] * s[0] + (s[1] * s[1] + s[2] * s[2] + s[3] * s[3]))
    return p1, tuple(x * n for x in s)


def derive_angular(q, past, h):
    """derive's angular velocity from the rotation a substep made: what a fixed body given a velocity is left with."""
    dr = qmul(q, (past[0], -past[1], -past[2], -past[3]))
    if dr[0] < 0.0:
        dr = tuple(-x for x in dr)
    return tuple((2.0 * x) / h for x in dr[1:])


def fly(p, q, entry, dt, substeps):
    """A kinematic body alone in space for one frame: [(position, rotation, velocity, angular_velocity)] after every substep, the
    velocities as derive leaves them."""
    h = dt / substeps
    out = []
    for k in range(substeps):
        row = np.zeros(38)
        row[POS], row[ROT] = p, q
        vel, ang = velocities(entry, row, h, substeps - k)
        past_p, past_q = p, q
        p, q = integrate_pose(p, q, vel, ang, h)
        out.append((p, q, tuple((p[c] - past_p[c]) / h for c in range(3)), derive_angular(q, past_q, h)))
    return out


def oracle_substeps(rows, sid, polys, joints, dt, substeps, pad, tbl=None):
    """One frame as `substeps` one-substep frames of the oracle, the table's overwrite before each.  Returns the rows."""
    h = dt / substeps
    b = np.array(rows, dtype=np.float64).reshape(-1, 38).copy()
    for k in range(substeps):
        if tbl is not None and len(tbl):
            b, _ = overwrite(b, tbl, h, substeps - k)
        b = ob.contacts_step_joints(b, sid, polys, joints, h, 1, pad)
    return b


def expected_frames(rows, sid, polys, joints, dt, substeps, pad, tables):
    """The rows after each of len(tables) frames; tables[f] is the kinematic table in force during frame f."""
    out, b = [], rows
    for tbl in tables:
        b = oracle_substeps(b, sid, polys, joints, dt, substeps, pad, tbl)
        out.append(b)
    return out
