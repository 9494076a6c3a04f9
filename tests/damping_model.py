"""Independent model of DAMPING (include/xpbd.h, "DAMPING") in plain Python floats, written from the header: stage 7 of a substep
-- joint dampers, drag, caps -- on the rows stage 6 left, and the expected frames of a world that has damping.

Python's float arithmetic is IEEE double, one rounding per operation and no contraction, and math.sqrt is correctly rounded:
exactly what the header asks for, so the GPU tests hold the device to this model bit for bit.

Stages 1 to 5 come from the committed oracle (oracle_binding.contacts_step_joints) run ONE SUBSTEP at a time, as
kinematic_model.py runs it, stage 6 from restitution_model.py when restitution is on (joint-free scenes, as that model), and
stage 7 is applied after each.  tests/test_damping_model.py shows first that the oracle run per substep equals the oracle run per
frame bit for bit on every scene used that way, and that this model with all defaults equals the oracle bit for bit."""
import math

import numpy as np

import oracle_binding as ob
from material_model import Body, add, cross, divs, dot, frame_mulv, inverse_resistance, lscale, magnitude, mat3_mulv, neg, qconj, qrot, scale, sub

INF = math.inf
VEL, ANG = slice(22, 25), slice(25, 28)
ROW_DTYPE = np.dtype([("linear", np.float64), ("angular", np.float64), ("max_linear_speed", np.float64), ("max_angular_speed", np.float64)])
JOINT_DAMPING_DTYPE = np.dtype([("joint", np.uint32), ("reserved", np.uint32), ("linear", np.float64), ("angular", np.float64)])
DEFAULT_ROW = (0.0, 0.0, INF, INF)


def rows(n, linear=0.0, angular=0.0, max_linear_speed=INF, max_angular_speed=INF):
    """n body rows; every argument a scalar or an array of n."""
    out = np.zeros(n, dtype=ROW_DTYPE)
    out["linear"], out["angular"], out["max_linear_speed"], out["max_angular_speed"] = linear, angular, max_linear_speed, max_angular_speed
    return out


def dampers(*entries):
    """entries: (joint, mu_l, mu_a)."""
    out = np.zeros(len(entries), dtype=JOINT_DAMPING_DTYPE)
    for k, (joint, mu_l, mu_a) in enumerate(entries):
        out[k]["joint"], out[k]["linear"], out[k]["angular"] = joint, mu_l, mu_a
    return out


class End(Body):
    """One end of a joint as stage 6 left it."""

    def __init__(self, row):
        super().__init__(row)
        self.vel = tuple(float(x) for x in row[VEL])
        self.ang = tuple(float(x) for x in row[ANG])

    def centre(self):
        return add(self.pos, self.com)

    def anchor(self, local):
        """Rigid::frame() at (x, q) times the anchor."""
        origin = add(self.centre(), qrot(self.rot, neg(self.com)))
        return frame_mulv((origin, self.rot), tuple(float(x) for x in local))


def is_fixed(row):
    return all(float(x) == 0.0 for x in row[0:10])


def share(mu, h):
    return mu * h if mu * h < 1.0 else 1.0


def joint_entry(a, b, joint, mu_l, mu_a, h):
    """The entries (dv, dw) of one joint for its end a and its end b, or None when no term acted."""
    zero = (0.0, 0.0, 0.0)
    ea, eb, terms = [zero, zero], [zero, zero], 0
    if mu_l > 0.0:
        p_a, p_b = a.anchor(joint["anchor_a"]), b.anchor(joint["anchor_b"])
        arm_a, arm_b = sub(p_a, a.centre()), sub(p_b, b.centre())
        d = sub(add(b.vel, cross(b.ang, arm_b)), add(a.vel, cross(a.ang, arm_a)))
        length = magnitude(d)
        if length != 0.0:
            n = scale(d, 1.0 / length)
            w_sum = inverse_resistance(a, p_a, n) + inverse_resistance(b, p_b, n)
            if w_sum > 0.0:
                lam = (share(mu_l, h) * length) / w_sum
                for e, body, arm, impulse in ((ea, a, arm_a, lscale(lam, n)), (eb, b, arm_b, lscale(-lam, n))):
                    e[0] = add(e[0], scale(impulse, body.inv_mass))
                    e[1] = add(e[1], cross(mat3_mulv(body.inv_inertia, arm), impulse))
                terms += 1
    if mu_a > 0.0:
        d = sub(b.ang, a.ang)
        length = magnitude(d)
        if length != 0.0:
            n = scale(d, 1.0 / length)
            n_a, n_b = qrot(qconj(a.rot), n), qrot(qconj(b.rot), n)
            w_ang = dot(mat3_mulv(a.inv_inertia, n_a), n_a) + dot(mat3_mulv(b.inv_inertia, n_b), n_b)
            if w_ang > 0.0:
                lam = (share(mu_a, h) * length) / w_ang
                for e, body, turn in ((ea, a, lscale(lam, n)), (eb, b, lscale(-lam, n))):
                    e[1] = add(e[1], qrot(body.rot, mat3_mulv(body.inv_inertia, qrot(qconj(body.rot), turn))))
                terms += 1
    return (ea, eb) if terms else None


def drag_and_cap(v, h, drag, cap):
    s = 1.0 / (1.0 + h * drag)
    v = scale(v, s)
    m = magnitude(v)
    if m > cap:
        v = scale(v, cap / m)
    return v


def stage7(state, joints, h, body_rows=None, joint_damping=None, asleep=None):
    """state ((n, 38) rows as stage 6 left them) after stage 7: a copy.  body_rows: ROW_DTYPE records or None (defaults);
    joint_damping: JOINT_DAMPING_DTYPE records or None; asleep: per-body flags or None (everybody awake)."""
    state = np.array(state, dtype=np.float64).reshape(-1, 38)
    out = state.copy()
    n = len(state)
    works = [not is_fixed(state[i]) and not (asleep is not None and asleep[i]) for i in range(n)]
    vel = [tuple(float(x) for x in state[i, VEL]) for i in range(n)]
    ang = [tuple(float(x) for x in state[i, ANG]) for i in range(n)]
    if joint_damping is not None and len(joint_damping):
        mu = {int(d["joint"]): (float(d["linear"]), float(d["angular"])) for d in joint_damping}
        zero = (0.0, 0.0, 0.0)
        sums = [[zero, zero, 0] for _ in range(n)]
        for j in range(len(joints)):                                  # ascending joint index: every body's own order
            mu_l, mu_a = mu.get(j, (0.0, 0.0))
            if not (mu_l > 0.0 or mu_a > 0.0):
                continue
            ia, ib = int(joints[j]["body_a"]), int(joints[j]["body_b"])
            entry = joint_entry(End(state[ia]), End(state[ib]), joints[j], mu_l, mu_a, h)
            if entry is None:
                continue
            for i, e in zip((ia, ib), entry):
                sums[i] = [add(sums[i][0], e[0]), add(sums[i][1], e[1]), sums[i][2] + 1]
        for i in range(n):
            dv, dw, count = sums[i]
            if works[i] and count:
                cnt = float(count)
                vel[i], ang[i] = add(vel[i], divs(dv, cnt)), add(ang[i], divs(dw, cnt))
    for i in range(n):
        if not works[i]:
            continue
        c_l, c_a, cap_l, cap_a = DEFAULT_ROW if body_rows is None else (float(x) for x in body_rows[i])
        out[i, VEL] = drag_and_cap(vel[i], h, c_l, cap_l)
        out[i, ANG] = drag_and_cap(ang[i], h, c_a, cap_a)
    return out


def oracle_substeps(state, sid, polys, joints, dt, substeps, pad, body_rows=None, joint_damping=None, narrowphase=0, on=True):
    """One frame as `substeps` one-substep frames of the oracle, stage 7 after each (on=False: the plain oracle per substep)."""
    h = dt / substeps
    b = np.array(state, dtype=np.float64).reshape(-1, 38).copy()
    for _ in range(substeps):
        b = ob.contacts_step_joints(b, sid, polys, joints, h, 1, pad, narrowphase=narrowphase)
        if on:
            b = stage7(b, joints, h, body_rows, joint_damping)
    return b


def restitution_substeps(model, dt, substeps, body_rows=None):
    """One frame of a restitution_model.Model (joint-free) as one-substep frames, stage 7 after each.  Returns its rows."""
    h = dt / substeps
    no_joints = np.zeros(0, dtype=np.dtype([("body_a", np.uint32), ("body_b", np.uint32)]))
    for _ in range(substeps):
        model.step(h, 1)
        model.bodies[:] = stage7(model.bodies, no_joints, h, body_rows)
    return model.bodies


def expected_frames(state, sid, polys, joints, dt, substeps, pad, frames, body_rows=None, joint_damping=None, narrowphase=0):
    """The rows after each of `frames` frames."""
    out, b = [], state
    for _ in range(frames):
        b = oracle_substeps(b, sid, polys, joints, dt, substeps, pad, body_rows, joint_damping, narrowphase)
        out.append(b)
    return out
