"""Independent model of the mass edits (include/xpbd.h, "MASS properties of resident bodies") in plain Python floats, written from
the header: the value rules of a row, the DIRECT inversion (Rigid::new: 1.0 / mass and cgmath's Matrix3::invert, determinant
first), the two KEEP_FRAME formulas, what a call makes of an xpbd_rigid array, and island sleeping in a world whose mass
properties change between frames (on top of sleep_model.py, which it does not touch).

Python's float is IEEE binary64 and CPython never fuses a multiply into an add, so every expression below rounds where the
header says it rounds and the comparison with the device is bit for bit."""
import math

import numpy as np

import sleep_model as sm

INVERSE, DIRECT, KEEP_FRAME = 0, 1, 0x100
OK, NOT_FINITE, NEGATIVE_INVERSE_MASS, MASS_NOT_POSITIVE, SINGULAR, KINEMATIC_RULE, OUT_OF_RANGE = range(7)

MASS_COLUMNS = list(range(0, 10)) + [28, 29, 30]          # the 13 mass doubles of an xpbd_rigid row, in the order of a row
COM, POS, ROT, VEL, ANG = slice(28, 31), slice(31, 34), slice(34, 38), slice(22, 25), slice(25, 28)


def cross(a, b):
    return ((a[1] * b[2]) - (a[2] * b[1]), (a[2] * b[0]) - (a[0] * b[2]), (a[0] * b[1]) - (a[1] * b[0]))


def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def scale(a, k):
    return (a[0] * k, a[1] * k, a[2] * k)


def neg(a):
    return (-a[0], -a[1], -a[2])


def qrot(q, v):
    """The rotation operator of Rigid::frame: t = qv x v + v * s;  (qv x t) * 2 + v."""
    qv = (q[1], q[2], q[3])
    t = add(cross(qv, v), scale(v, q[0]))
    return add(scale(cross(qv, t), 2), v)


def frame_origin(pos, rot, com):
    """Rigid::frame().position: (position + com) + rotation * (-com)."""
    return add(add(pos, com), qrot(rot, neg(com)))


def invert(m):
    """cgmath's Matrix3::invert of the columns m = (x, y, z): None when the determinant is 0, else the three columns."""
    x, y, z = m
    det = (x[0] * (y[1] * z[2] - z[1] * y[2]) - y[0] * (x[1] * z[2] - z[1] * x[2])) + z[0] * (x[1] * y[2] - y[1] * x[2])
    if det == 0.0:
        return None
    r0 = tuple(c / det for c in cross(y, z))
    r1 = tuple(c / det for c in cross(z, x))
    r2 = tuple(c / det for c in cross(x, y))
    return ((r0[0], r1[0], r2[0]), (r0[1], r1[1], r2[1]), (r0[2], r1[2], r2[2]))


def resolve(row, layout):
    """(verdict, the 13 doubles the body takes or None) of one row, by the header's rules in the header's order."""
    row = [float(v) for v in row]
    if not all(math.isfinite(v) for v in row):
        return NOT_FINITE, None
    if layout == INVERSE:
        if row[0] < 0.0:
            return NEGATIVE_INVERSE_MASS, None
        return OK, row
    if not row[0] > 0.0:
        return MASS_NOT_POSITIVE, None
    inv = invert((tuple(row[1:4]), tuple(row[4:7]), tuple(row[7:10])))
    if inv is None:
        return SINGULAR, None
    return OK, [1.0 / row[0]] + list(inv[0]) + list(inv[1]) + list(inv[2]) + row[10:13]


def is_fixed(out):
    return all(v == 0.0 for v in out[:10])


def keep_frame(pos, rot, vel, ang, com, com_new):
    """(position', velocity') of the two KEEP_FRAME formulas."""
    d = sub(com_new, com)
    r = qrot(rot, d)
    return add(pos, sub(r, d)), add(vel, cross(ang, r))


def apply(bodies, indices, rows, flags, kinematic=()):
    """What the DEVICE variant makes of an xpbd_rigid array ((n, 38)): (the array afterwards, the verdict of every entry).  An
    entry with a verdict other than OK is skipped.  The host variant applies the same when every verdict is OK and refuses the
    whole call otherwise.  kinematic: the bodies that have an entry in the kinematic table."""
    b = np.array(bodies, dtype=np.float64).reshape(-1, 38).copy()
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 13)
    idx = range(len(rows)) if indices is None else [int(i) for i in indices]
    verdicts = []
    for k, i in enumerate(idx):
        if i >= len(b):
            verdicts.append(OUT_OF_RANGE)
            continue
        verdict, out = resolve(rows[k], flags & 0xFF)
        if verdict == OK and i in kinematic and not is_fixed(out):
            verdict = KINEMATIC_RULE
        verdicts.append(verdict)
        if verdict != OK:
            continue
        if flags & KEEP_FRAME:
            p, v = keep_frame(tuple(b[i, POS]), tuple(b[i, ROT]), tuple(b[i, VEL]), tuple(b[i, ANG]), tuple(b[i, COM]), tuple(out[10:13]))
            b[i, POS], b[i, VEL] = p, v
        b[i, MASS_COLUMNS] = out
    return b, verdicts


def sleep_frame(state, bodies, pairs, joints, cfg, named=(), fixed_when_named=None, wake_all=False):
    """One xpbd_world_step of a world with sleeping on, sleep_model.frame with one difference: a request is judged by the mass
    properties its body had WHEN IT WAS NAMED (fixed_when_named[n]: before the mass edit), while the pass itself sees the bodies
    as the frame left them -- a sleeper made fixed wakes its group and is inert from then on, a fixed body released wakes all."""
    import islands_model as im
    fixed = im.fixed_bodies(bodies) if fixed_when_named is None else fixed_when_named
    begun = sm.frame_begin(state, fixed, sm.Requests(bodies=named, wake_all=wake_all))
    return sm.sleep_pass(begun, bodies, pairs, joints, *cfg)
