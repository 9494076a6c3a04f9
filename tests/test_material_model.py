"""The model of contact materials (tests/material_model.py) on the CPU: first that it is a faithful restatement of the
oracle's contact pipeline (every coefficient +inf: bit for bit), then what friction does in it -- a box on a slope sticks or
slides, its sliding acceleration against Coulomb's closed form, and a frictionless ground pushes straight up.

The slope is made by tilting gravity through external_force (the ground stays z = 0): with theta the slope angle, the force
on a body of mass m is m g (sin theta, 0, -cos theta)."""
import math

import numpy as np
import pytest

import material_model as mm
import oracle_binding as ob
from constraint_solver_amd import capi
from golden_util import bits_equal
from halo_common import POLY_NAMES, pile

DT = 1.0 / 60.0
G = 9.81


def slide(tan_theta, mu, frames, substeps=20, ground_mu=mm.INF):
    """x of the box after every frame."""
    bodies, sid, theta = mm.resting_box(capi, tan_theta)
    model = mm.Model(bodies, sid, ob.polytopes_array(POLY_NAMES[capi.SCENE_BOXES]), [mu], ground_mu)
    xs = [float(model.bodies[0, 31])]
    for _ in range(frames):
        model.step(DT, substeps)
        xs.append(float(model.bodies[0, 31]))
    return np.array(xs), theta, model


# ---- faithful: all coefficients +inf is the oracle, bit for bit ---------------------------------------------------------
@pytest.mark.parametrize("speed", [0.0, 3.0])
@pytest.mark.parametrize("kind,n,seed", [(capi.SCENE_BOXES_DROP, 40, 3), (capi.SCENE_MIXED_DROP, 48, 5)])
def test_model_with_infinite_friction_is_the_oracle(kind, n, seed, speed):
    bodies, sid = pile(capi, kind, n, seed, 3.0, 2.5)          # interpenetrating: ground and pair contacts from frame 0
    polys = ob.polytopes_array(POLY_NAMES[kind])
    model = mm.Model(bodies, sid, polys, None, mm.INF, pad=0.02, max_depenetration_speed=speed)
    want = bodies
    stats = ob.ContactStats()
    ground = 0
    for _ in range(12):
        model.ground_trace = []
        got = model.step(DT, 6)
        ground += len(model.ground_trace)
        want = ob.contacts_step_joints(want, sid, polys, np.zeros(0, dtype=capi.JOINT_DTYPE), DT, 6, 0.02, stats=stats,
                                       max_depenetration_speed=speed)
        assert bits_equal(got, want)
    assert not np.isnan(want).any()
    assert stats.n_points > 50 and ground > 50                 # both contact kinds took part (a check of the scene)


def test_explicit_infinite_coefficients_equal_none():
    bodies, sid = pile(capi, capi.SCENE_BOXES_DROP, 24, 2, 2.5, 2.0)
    polys = ob.polytopes_array(POLY_NAMES[capi.SCENE_BOXES_DROP])
    a = mm.Model(bodies, sid, polys)
    b = mm.Model(bodies, sid, polys, [mm.INF] * 24, mm.INF)
    for _ in range(3):
        assert bits_equal(a.step(DT, 5), b.step(DT, 5))


# ---- slope --------------------------------------------------------------------------------------------------------------
def test_box_on_a_gentle_slope_stays_put():
    """It does creep: the contact is compliant, 1e-6 / h^2, and the four corners are projected one after the other.  Measured:
    3.7 mm/s at mu = 0.5, 1.3 mm/s at mu = +inf, 49 mm in the first second at mu = 0.24 -- just below tan(theta) -- where
    Coulomb gives 48 mm; a frictionless box covers 1.19 m."""
    xs, theta, _ = slide(0.25, 0.5, 60)
    free = 0.5 * G * math.sin(theta)
    print("gentle slope: moved %.3e m of %.3f m" % (xs[-1] - xs[0], free))
    assert abs(xs[-1] - xs[0]) < mm.STICKS * free


def test_box_on_a_steep_slope_slides():
    xs, theta, _ = slide(1.0, 0.5, 60)
    free = 0.5 * G * math.sin(theta)                            # the frictionless distance after one second: 3.47 m
    print("steep slope: moved %.4f m of %.3f m" % (xs[-1] - xs[0], free))
    assert mm.SLIDES * free < xs[-1] - xs[0] < (1.0 - mm.SLIDES) * free   # Coulomb: (1 - mu / tan(theta)) = half of it


def test_box_on_a_static_slab_sticks_slides_and_takes_the_smaller_coefficient():
    """The same through the pair contacts: the box rests on a static body (material_model.box_on_slab), half a second."""
    polys = (ob.Polytope * 2)(ob.polytope("cube", 1.0), ob.polytope("cube", 4.0))
    for tan_theta, mus, verdict in ((0.25, [0.5, 0.5], 'sticks'), (1.0, [0.5, 0.5], 'slides'), (0.5, [0.0, 1.0], 'free'), (0.5, [1.0, 0.0], 'free'),
                                   (0.5, [1.0, 1.0], 'sticks')):
        bodies, sid, theta, _ = mm.box_on_slab(capi, tan_theta)
        model = mm.Model(bodies, sid, polys, mus)
        for _ in range(30):
            model.step(DT, 20)
        moved, free = model.bodies[0, 31] - bodies[0, 31], 0.5 * G * math.sin(theta) * 0.25
        print("slab: tan(theta) %.2f mu %s moved %.4f m of %.4f m" % (tan_theta, mus, moved, free))
        assert bits_equal(model.bodies[1], bodies[1])             # the slab does not move
        if verdict == 'sticks':
            assert abs(moved) < mm.STICKS * free
        elif verdict == 'slides':
            assert mm.SLIDES * free < moved < (1.0 - mm.SLIDES) * free
        else:                                                   # min(0, 1) = 0: frictionless
            assert moved > (1.0 - mm.STICKS) * free


def test_friction_of_the_ground_counts_too():
    """mu = min(body, ground): a sticky box on an icy ground slides, and so does an icy box on a sticky ground."""
    for mu_body, mu_ground in ((1e9, 0.0), (0.0, 1e9)):
        xs, theta, _ = slide(0.25, mu_body, 60, ground_mu=mu_ground)
        assert xs[-1] - xs[0] > 0.9 * 0.5 * G * math.sin(theta)


# ---- rate ---------------------------------------------------------------------------------------------------------------
# Sliding acceleration against Coulomb's closed form a = g (sin theta - mu cos theta), tan theta = 1, mu = 0.5, fitted to the
# positions of frames 30..90 of a box started at rest (20 substeps).  MEASURED on the CPU model before the bound was chosen:
# 3.4683587619 m/s^2 against 3.4683587617, a relative deviation of 4.5e-11.  (Why so small: per substep the normal correction
# is len_c = h^2 g cos(theta) and the contact takes back mu * len_c of the slip, which is Coulomb's law exactly; what is left
# is rounding and the fit.)  Other fit windows gave 2.0e-12 (frames 10..60) and 1.4e-10 (60..120); mu = 0.2 gave 5.9e-11 and
# tan(theta) = 0.75 gave 3.3e-11.  With 5 / 10 / 40 substeps the deviation is 1.2e-5 / 5.0e-6 / 2.4e-10.
# The asserted bound is 1e-9: about 20 times the measurement, 7 times the worst window.
RATE_MEASURED = 4.5e-11
RATE_BOUND = 1e-9


def sliding_acceleration(tan_theta, mu, first=30, last=90):
    xs, theta, _ = slide(tan_theta, mu, last)
    t = np.arange(first, last + 1) * DT
    a2, _, _ = np.polyfit(t, xs[first:last + 1], 2)
    return 2.0 * a2, G * (math.sin(theta) - mu * math.cos(theta))


def test_sliding_acceleration_against_coulomb():
    got, want = sliding_acceleration(1.0, 0.5)
    deviation = abs(got - want) / want
    print("sliding acceleration: model %.6f, closed form %.6f, relative deviation %.3e" % (got, want, deviation))
    assert deviation < RATE_BOUND


# ---- frictionless ---------------------------------------------------------------------------------------------------------
def test_frictionless_ground_pushes_straight_up():
    bodies, sid, _ = mm.resting_box(capi, 1.0)
    bodies[0, 22:25] = [0.7, -0.4, 0.0]                         # and it slides along
    model = mm.Model(bodies, sid, ob.polytopes_array(POLY_NAMES[capi.SCENE_BOXES]), [0.0], 1.0)
    model.ground_trace = []
    for _ in range(5):
        model.step(DT, 20)
    assert len(model.ground_trace) >= 4 * 50
    for _, direction, impulse in model.ground_trace:
        assert direction[0] == 0.0 and direction[1] == 0.0 and direction[2] > 0.0
        assert impulse[0] == 0.0 and impulse[1] == 0.0
