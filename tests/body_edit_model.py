"""Body edits (include/xpbd.h, "Body EDITS") in plain Python floats: the impulse arithmetic of xpbd_world_apply_impulses,
operation for operation, on rows of the xpbd_rigid array.  IEEE doubles without contraction, so the device must give the same
bits.  The vector algebra is material_model's (cgmath's operation order), as in restitution_model."""
import numpy as np

from material_model import add, cross, mat3_mulv, scale, sub

AT_POINT, AT_CENTRE = 0, 1


def _vec(row, first):
    return tuple(float(x) for x in row[first:first + 3])


def apply_impulse(row, impulse, point, angular_impulse, flags):
    """One entry on one xpbd_rigid row (38 doubles), in place: velocity and angular_velocity change, nothing else."""
    inv_mass = float(row[0])
    inv_inertia = (_vec(row, 1), _vec(row, 4), _vec(row, 7))      # three columns
    centre = add(_vec(row, 31), _vec(row, 28))                    # position + center_of_mass
    vel, ang = _vec(row, 22), _vec(row, 25)
    impulse, angular_impulse = tuple(float(x) for x in impulse), tuple(float(x) for x in angular_impulse)
    vel = add(vel, scale(impulse, inv_mass))
    if not flags & AT_CENTRE:
        arm = sub(tuple(float(x) for x in point), centre)
        ang = add(ang, cross(mat3_mulv(inv_inertia, arm), impulse))
    ang = add(ang, mat3_mulv(inv_inertia, angular_impulse))
    row[22:25], row[25:28] = vel, ang


def apply_impulses(bodies, entries):
    """A copy of `bodies` ((n, 38)) after the entries (records with body, flags, impulse, point, angular_impulse) in list
    order: the entries of one body one after another, each on the result of the one before."""
    out = np.array(bodies, dtype=np.float64).reshape(-1, 38).copy()
    for e in entries:
        apply_impulse(out[int(e["body"])], e["impulse"], e["point"], e["angular_impulse"], int(e["flags"]))
    return out
