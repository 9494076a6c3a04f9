"""The CPU model of xpbd_world_apply_impulses against answers worked out by hand for a unit box."""
import numpy as np

import body_edit_model as bm

IMPULSE = np.dtype([("body", "<u4"), ("flags", "<u4"), ("impulse", "<f8", (3,)), ("point", "<f8", (3,)), ("angular_impulse", "<f8", (3,))])


def unit_box(mass=2.0):
    """A 1 m cube of `mass` kg: inertia m / 6 about every axis, corner at the origin, centre of mass at its middle."""
    row = np.zeros(38)
    row[0] = 1.0 / mass
    row[1], row[5], row[9] = (6.0 / mass,) * 3
    row[28:31] = 0.5
    row[31:34] = [10.0, 20.0, 30.0]
    row[34] = 1.0
    row[22:25] = [1.0, 0.0, -1.0]
    row[25:28] = [0.0, 0.25, 0.0]
    return row


def entry(body=0, flags=bm.AT_POINT, impulse=(0, 0, 0), point=(0, 0, 0), angular=(0, 0, 0)):
    e = np.zeros(1, dtype=IMPULSE)
    e["body"], e["flags"], e["impulse"], e["point"], e["angular_impulse"] = body, flags, impulse, point, angular
    return e[0]


def test_impulse_at_the_centre_changes_only_the_velocity():
    box = unit_box()
    # the point is garbage on purpose: AT_CENTRE ignores it
    out = bm.apply_impulses([box], [entry(flags=bm.AT_CENTRE, impulse=(4.0, -2.0, 6.0), point=(np.nan, 1e300, -7.0))])[0]
    assert list(out[22:25]) == [1.0 + 2.0, 0.0 - 1.0, -1.0 + 3.0]          # P / m, m = 2
    assert list(out[25:28]) == [0.0, 0.25, 0.0]
    rest = np.r_[0:22, 28:38]
    assert out[rest].tobytes() == box[rest].tobytes()


def test_impulse_through_the_centre_given_as_a_point_adds_no_spin():
    box = unit_box()
    out = bm.apply_impulses([box], [entry(impulse=(4.0, 0.0, 0.0), point=(10.5, 20.5, 30.5))])[0]
    assert list(out[22:25]) == [3.0, 0.0, -1.0]
    assert list(out[25:28]) == [0.0, 0.25, 0.0]


def test_impulse_at_an_offset_point_spins_the_box():
    box = unit_box()
    # arm = (0, 0.5, 0) from the centre (10.5, 20.5, 30.5); P = (4, 0, 0); I^-1 = 3:  dw = (3 * arm) x P = (0, 1.5, 0) x (4, 0, 0)
    out = bm.apply_impulses([box], [entry(impulse=(4.0, 0.0, 0.0), point=(10.5, 21.0, 30.5))])[0]
    assert list(out[22:25]) == [3.0, 0.0, -1.0]
    assert list(out[25:28]) == [0.0, 0.25, -6.0]


def test_angular_impulse_gives_inverse_inertia_times_it():
    box = unit_box()
    out = bm.apply_impulses([box], [entry(flags=bm.AT_CENTRE, angular=(1.0, -2.0, 0.5))])[0]
    assert list(out[22:25]) == [1.0, 0.0, -1.0]
    assert list(out[25:28]) == [3.0, 0.25 - 6.0, 1.5]


def test_static_body_keeps_its_velocities():
    box = unit_box()
    box[0:10] = 0.0
    out = bm.apply_impulses([box], [entry(impulse=(4.0, 5.0, 6.0), point=(0.0, 0.0, 0.0), angular=(1.0, 1.0, 1.0))])[0]
    assert out.tobytes() == box.tobytes()


def test_two_entries_on_one_body_are_applied_one_after_the_other():
    rng = np.random.default_rng(5)
    box = unit_box(mass=3.7)
    box[1:10] = rng.normal(size=9)              # any matrix: the model is arithmetic, not physics
    other = unit_box(mass=0.3)
    a = entry(impulse=rng.normal(size=3), point=rng.normal(size=3) + 10.0, angular=rng.normal(size=3))
    b = entry(flags=bm.AT_CENTRE, impulse=rng.normal(size=3), angular=rng.normal(size=3))
    c = entry(body=1, impulse=(1.0, 2.0, 3.0), point=(10.0, 20.0, 30.0))
    both = bm.apply_impulses([box, other], [a, c, b])
    step = bm.apply_impulses(bm.apply_impulses([box, other], [a]), [b])
    assert both[0].tobytes() == step[0].tobytes()
    assert both[1].tobytes() == bm.apply_impulses([box, other], [c])[1].tobytes()
    swapped = bm.apply_impulses([box, other], [b, c, a])
    assert swapped[1].tobytes() == both[1].tobytes()           # entries of different bodies are independent
