"""Independent model of xpbd_world_joint_states: the eight quantities and the flags of a joint from downloaded body rows.

Written from include/xpbd.h ("Joint STATES and drive TARGETS") in Python floats, not from the kernel.  The angles are those of
the existing models (limit_angle of tests/joint_limit_model.py, hinge_angle and slide_offset of tests/joint_drive_model.py);
the rates, the flags and the choice of references are this file's own.  Its operation order is its own and atan2 is the
host's, so it agrees with the device to rounding, not bit for bit.

A body is a row of 38 doubles (xpbd_rigid); joints, limits and drives are numpy records with the field names of
capi.JOINT_DTYPE / JOINT_LIMIT_DTYPE / JOINT_DRIVE_DTYPE (no device library is needed).
"""
import math

import numpy as np

from joint_drive_model import (DRIVE_ANGLE, DRIVE_ANGULAR_VELOCITY, JOINT_DISTANCE, JOINT_SLIDER, LIMIT_HINGE, LIMIT_SLIDE, LIMIT_SWING, LIMIT_TWIST,
                               hinge_angle, slide_offset)
from joint_limit_model import Body, _norm, limit_angle
from xprec_model import cross, dot, qrot

STATE_DTYPE = np.dtype([("separation", "<f8"), ("misalignment", "<f8"), ("angle", "<f8"), ("angle_rate", "<f8"), ("travel", "<f8"),
                        ("travel_rate", "<f8"), ("swing", "<f8"), ("twist", "<f8"), ("joint", "<u4"), ("kind", "<u4"), ("flags", "<u4"),
                        ("reserved", "<u4")])
DOUBLES = ["separation", "misalignment", "angle", "angle_rate", "travel", "travel_rate", "swing", "twist"]
HAS_ANGLE, HAS_TRAVEL, HAS_SWING, HAS_TWIST, ANGLE_OF_DRIVE = 0x001, 0x002, 0x004, 0x008, 0x010
ANGLE_BELOW, ANGLE_ABOVE, TRAVEL_BELOW, TRAVEL_ABOVE, SWING_ABOVE, TWIST_BELOW, TWIST_ABOVE = 0x100, 0x200, 0x400, 0x800, 0x1000, 0x2000, 0x4000


def _point_velocity(body, p):
    """velocity + angular_velocity x (p - (position + center_of_mass)), angular_velocity in world space"""
    return body.vel + cross(body.ang, p - (body.pos + body.com))


def _side(value, lower, upper, below, above):
    return below if value < lower else (above if value > upper else 0)


def joint_state(rows, index, joint, limits, drives):
    """The state of one joint as a dict of the eight doubles, `joint`, `kind`, `flags`, plus `margins`: the distance of every
    reported angle or travel to each bound it was compared with (what a test checks before it trusts the limit bits).
    limits, drives: those of this joint, the caller's order."""
    a, b = Body(rows[int(joint["body_a"])]), Body(rows[int(joint["body_b"])])
    kind = int(joint["kind"])
    out = dict.fromkeys(DOUBLES, 0.0)
    flags, margins = 0, []
    s, d, a_w, p_a, p_b = slide_offset(joint, a, b)
    b_w = qrot(b.rot, np.asarray(joint["axis_b"], dtype=np.float64))
    if kind == JOINT_SLIDER:
        out["separation"] = _norm(d - a_w * s)
        out["travel"] = float(s)
        out["travel_rate"] = float(dot(_point_velocity(b, p_b) - _point_velocity(a, p_a), a_w) + dot(d, cross(a.ang, a_w)))
        flags |= HAS_TRAVEL
    else:
        out["separation"] = _norm(d) - float(joint["distance"])
    if kind != JOINT_DISTANCE:
        out["misalignment"] = _norm(cross(a_w, b_w))
    refs = None
    for drv in drives:
        if int(drv["kind"]) in (DRIVE_ANGLE, DRIVE_ANGULAR_VELOCITY):
            refs = (drv["ref_a"], drv["ref_b"])
            flags |= ANGLE_OF_DRIVE
    swing_wanted = False
    for lim in limits:
        lk, lower, upper = int(lim["kind"]), float(lim["lower"]), float(lim["upper"])
        if lk == LIMIT_SLIDE:
            flags |= _side(s, lower, upper, TRAVEL_BELOW, TRAVEL_ABOVE)
            margins += [abs(s - lower), abs(s - upper)]
        elif lk == LIMIT_HINGE:
            phi = hinge_angle(joint, lim["ref_a"], lim["ref_b"], a.rot, b.rot)
            flags |= _side(phi, lower, upper, ANGLE_BELOW, ANGLE_ABOVE)
            margins += [abs(phi - lower), abs(phi - upper)]
            if refs is None:
                refs = (lim["ref_a"], lim["ref_b"])
        elif lk == LIMIT_SWING:
            swing_wanted = True
            got = limit_angle(LIMIT_SWING, a.rot, b.rot, joint["axis_a"], joint["axis_b"], None, None)
            if got is not None:
                flags |= _side(got[0], -math.inf, upper, 0, SWING_ABOVE)
                margins.append(abs(got[0] - upper))
        elif lk == LIMIT_TWIST:
            swing_wanted = True
            got = limit_angle(LIMIT_TWIST, a.rot, b.rot, joint["axis_a"], joint["axis_b"], lim["ref_a"], lim["ref_b"])
            if got is not None:
                out["twist"] = got[0]
                flags |= HAS_TWIST | _side(got[0], lower, upper, TWIST_BELOW, TWIST_ABOVE)
                margins += [abs(got[0] - lower), abs(got[0] - upper)]
        else:
            raise ValueError("unknown limit kind %r" % lk)
    if swing_wanted:
        out["swing"] = math.atan2(_norm(cross(a_w, b_w)), dot(a_w, b_w))
        flags |= HAS_SWING
    if refs is not None:
        out["angle"] = hinge_angle(joint, refs[0], refs[1], a.rot, b.rot)
        out["angle_rate"] = float(dot(b.ang - a.ang, a_w))
        flags |= HAS_ANGLE
    out.update(joint=index, kind=kind, flags=flags, margins=margins)
    return out


def joint_states(rows, joints, limits, drives, which=None):
    """(STATE_DTYPE records, smallest margin) of the joints `which` (None: all), as xpbd_world_joint_states reports them."""
    rows = np.asarray(rows, dtype=np.float64).reshape(-1, 38)
    lim_of = [[] for _ in range(len(joints))]
    drv_of = [[] for _ in range(len(joints))]
    for lim in limits:
        lim_of[int(lim["joint"])].append(lim)
    for drv in drives:
        drv_of[int(drv["joint"])].append(drv)
    which = range(len(joints)) if which is None else [int(k) for k in which]
    out = np.zeros(len(which), dtype=STATE_DTYPE)
    margin = math.inf
    for row, k in zip(out, which):
        st = joint_state(rows, k, joints[k], lim_of[k], drv_of[k])
        for name in DOUBLES + ["joint", "kind", "flags"]:
            row[name] = st[name]
        margin = min([margin] + st["margins"])
    return out, margin
