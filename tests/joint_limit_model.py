"""Independent model of XPBD_MODE_CONTACTS for jointed bodies that touch nothing: no ground contact, no two bodies'
bounding shapes overlapping.  One substep is integrate, the Jacobi joint pass (positional term, hinge term, angular
limits) and derive.

Written from include/xpbd.h (XPBD_JOINT_*, XPBD_LIMIT_*) in plain f64 numpy, not from the kernels and without calling
oracle/.  The integrate and derive stages are those of tests/xprec_model.py (the reference's Rigid::integrate and
Rigid::derive) evaluated in f64.  Its operation order is its own, so it agrees with the device to rounding, not bit for
bit; the device's f64 atan2 is not correctly rounded either.

A body is a row of 38 doubles (xpbd_rigid); joints and limits are numpy records of capi.JOINT_DTYPE / JOINT_LIMIT_DTYPE.
"""
import numpy as np

from xprec_model import conj, cross, dot, matvec, qmul, qrot

JOINT_HINGE = 1
LIMIT_HINGE, LIMIT_SWING, LIMIT_TWIST = 0, 1, 2


def _norm(v):
    return float(np.sqrt(dot(v, v)))


def _normalized_q(q):
    return q / np.sqrt(q[0] * q[0] + dot(q[1:], q[1:]))


def _pure(v):
    return np.concatenate([[0.0], v])


class Body:
    """The pose of one body during a substep, with its mass properties."""

    def __init__(self, row):
        row = np.asarray(row, dtype=np.float64)
        self.im = row[0]
        self.M = row[1:10].reshape(3, 3)           # [column, row]: matvec(M, v) = I^-1 v
        self.ef, self.fi, self.et, self.ti = row[10:13], row[13:16], row[16:19], row[19:22]
        self.vel, self.ang, self.com = row[22:25].copy(), row[25:28].copy(), row[28:31]
        self.pos, self.rot = row[31:34].copy(), row[34:38].copy()

    def point(self, anchor):
        """Frame * anchor: rotation * anchor + the frame's origin pos + com - rotation * com."""
        return qrot(self.rot, np.asarray(anchor, dtype=np.float64)) + self.pos + self.com + qrot(self.rot, -self.com)

    def angular_w(self, n):
        m = qrot(conj(self.rot), n)
        return dot(matvec(self.M, m), m)


def limit_angle(kind, q_a, q_b, axis_a, axis_b, ref_a, ref_b):
    """(phi, n) of a limit for the body rotations q_a, q_b (xpbd.h), or None where the limit defines no entry."""
    a_w = qrot(q_a, np.asarray(axis_a, dtype=np.float64))
    b_w = qrot(q_b, np.asarray(axis_b, dtype=np.float64))
    if kind == LIMIT_SWING:
        c = cross(a_w, b_w)
        s = _norm(c)
        if s == 0.0:
            return None
        return float(np.arctan2(s, dot(a_w, b_w))), c / s
    r_a = qrot(q_a, np.asarray(ref_a, dtype=np.float64))
    r_b = qrot(q_b, np.asarray(ref_b, dtype=np.float64))
    if kind == LIMIT_HINGE:
        n = a_w
    elif kind == LIMIT_TWIST:
        bis = a_w + b_w
        length = _norm(bis)
        if length == 0.0:
            return None
        n = bis / length
        r_a = r_a - n * dot(r_a, n)
        r_b = r_b - n * dot(r_b, n)
    else:
        raise ValueError("unknown limit kind %r" % kind)
    return float(np.arctan2(dot(cross(r_a, r_b), n), dot(r_a, r_b))), n


def _angular_entry(a, b, n, lam_numerator, compliance):
    """The turns (of a, of b) of one angular Jacobi entry with axis n and error lam_numerator."""
    lam = lam_numerator / (a.angular_w(n) + b.angular_w(n) + compliance)
    return lam * n, -lam * n


def _joint_entries(bodies, joint, limits, compliance):
    """Every Jacobi entry of one joint in order: a list of (body, dpos, turn-or-None, arm-impulse-or-None)."""
    ia, ib = int(joint["body_a"]), int(joint["body_b"])
    a, b = bodies[ia], bodies[ib]
    out = []
    p_a, p_b = a.point(joint["anchor_a"]), b.point(joint["anchor_b"])
    diff = p_b - p_a
    dist = _norm(diff)
    if dist != 0.0:
        d = diff / dist
        w = 0.0
        for body, p in ((a, p_a), (b, p_b)):
            r = qrot(conj(body.rot), cross(p - (body.pos + body.com), d))
            w += body.im + dot(matvec(body.M, r), r)
        lam = (dist - float(joint["distance"])) / (w + compliance)
        # Rigid::apply_impulse: dpos = impulse * m^-1, spin = (I^-1 arm) x impulse with the world-space arm
        out.append((ia, lam * d * a.im, cross(matvec(a.M, p_a - (a.pos + a.com)), lam * d)))
        out.append((ib, -lam * d * b.im, cross(matvec(b.M, p_b - (b.pos + b.com)), -lam * d)))
    if int(joint["kind"]) == JOINT_HINGE:
        a_w, b_w = qrot(a.rot, joint["axis_a"]), qrot(b.rot, joint["axis_b"])
        delta = cross(a_w, b_w)
        mag = _norm(delta)
        if mag != 0.0:
            ta, tb = _angular_entry(a, b, delta / mag, mag, compliance)
            out.append((ia, np.zeros(3), matvec(a.M, ta)))
            out.append((ib, np.zeros(3), matvec(b.M, tb)))
    for lim in limits:
        got = limit_angle(int(lim["kind"]), a.rot, b.rot, joint["axis_a"], joint["axis_b"], lim["ref_a"], lim["ref_b"])
        if got is None:
            continue
        phi, n = got
        err = phi - min(max(phi, float(lim["lower"])), float(lim["upper"]))
        if err == 0.0:
            continue
        ta, tb = _angular_entry(a, b, n, err, compliance)
        out.append((ia, np.zeros(3), matvec(a.M, ta)))
        out.append((ib, np.zeros(3), matvec(b.M, tb)))
    return out


def substep(rows, joints, limits, h):
    """One substep of (n, 38) f64 body rows; returns the new rows."""
    rows = np.array(rows, dtype=np.float64).reshape(-1, 38)
    bodies = [Body(r) for r in rows]
    compliance = 1e-6 / (h * h)
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
    by_joint = [[] for _ in range(len(joints))]
    for lim in limits:
        by_joint[int(lim["joint"])].append(lim)
    for k, joint in enumerate(joints):
        for i, dp, spin in _joint_entries(bodies, joint, by_joint[k], compliance):
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


def step(rows, joints, limits, dt, substeps):
    """xpbd_world_step(dt, substeps) of the model."""
    h = dt / substeps
    for _ in range(substeps):
        rows = substep(rows, joints, limits, h)
    return rows
