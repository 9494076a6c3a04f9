"""Known answers for the model of sliders and joint drives alone (tests/joint_drive_model.py): before the device is held
to the model, the model is held to mechanics.  Every bound below is worked out from the step's own discretisation (noted at
the bound), none from what the model returns.  No device, no library: plain numpy."""
import math

import numpy as np
import pytest

import joint_drive_model as jd
import joint_limit_model as jm

H20 = jd.DT / 20                                       # the substep of the 20-substep scenes
ULP_POS = np.spacing(26.0)                             # positions in these scenes stay below 26 m


@pytest.fixture(scope="module")
def paths():
    return {name: jd.run_scene(name) for name in set(jd.FIGURES.values())}


def figure(paths, name):
    value, answer = jd.measure(name, paths[jd.FIGURES[name]])
    print("%s: model %.17g, known answer %.17g, deviation %.3g" % (name, value, answer, value - answer))
    return float(value), answer


def velocity_noise(steps):
    """derive() reads a velocity off two positions, each rounded to an ulp of its size, and the next integrate starts from that
    velocity: at worst one ulp / h more per substep."""
    return steps * ULP_POS / H20


def test_without_extras_the_model_is_the_limits_model():
    """Hinge and ball joints with angular limits only: the same entries as tests/joint_limit_model.py, to rounding."""
    rng = np.random.default_rng(5)
    rows = np.zeros((3, 38))
    rows[:, 0], rows[:, 34] = 1.0, 1.0
    rows[:, [1, 5, 9]] = 6.0
    rows[:, 28:31] = 0.5
    rows[:, 31] = [0.0, 2.0, 4.0]
    rows[:, 33] = 9.0
    rows[:, 22:28] = rng.normal(size=(3, 6))
    joints = np.zeros(2, dtype=jd.JOINT_DTYPE)
    joints["body_a"], joints["body_b"], joints["kind"] = [0, 1], [1, 2], [jd.JOINT_HINGE, jd.JOINT_DISTANCE]
    joints["anchor_a"], joints["anchor_b"] = [1.5, 0.5, 0.5], [-0.5, 0.5, 0.5]
    joints["axis_a"] = joints["axis_b"] = jd.Z
    limits = jd.records(jd.LIMIT_DTYPE, dict(joint=0, kind=jd.LIMIT_HINGE, ref_a=jd.X, ref_b=jd.X, lower=-0.01, upper=0.01),
                        dict(joint=1, kind=jd.LIMIT_SWING, upper=0.01))
    want = jm.step(rows, joints, limits, jd.DT, 20)
    got = jd.step(rows, joints, limits, jd.NO_DRIVES, jd.DT, 20)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)


def test_velocity_drive_turns_a_free_wheel_at_its_speed(paths):
    """The drive asks for speed * h of TRUE angle per substep.  What is left to it each substep is the defect of the quaternion
    integrate / derive pair, which turns a body by 2 atan(sin(x / 2)) where its last substep turned it by x = speed * h: short by
    x^3 / 8.  So the speed read off the angle is short by less than speed * x^2 / 8."""
    value, answer = figure(paths, "wheel")
    assert abs(value - answer) <= answer * (answer * H20) ** 2 / 8
    assert value != answer                                              # (the bound is not met by standing still at the answer)
    last = paths["wheel"][-1]
    assert np.abs(last[1, 25:27]).max() == 0.0 and np.array_equal(last[0], jd.scene("wheel")[0][0])


def test_angle_drive_with_compliance_is_a_torsion_spring(paths):
    """At rest the drive's torque balances the load: torque = (phi - target) / (compliance + 1e-6), the 1e-6 being the solver's
    own regularisation.  The answer of the ideal spring is therefore missed by torque * 1e-6; twice that allows for what is left
    of the oscillation after 200 substeps."""
    value, answer = figure(paths, "spring")
    assert abs(value - answer) <= 2 * jd.SPRING_TORQUE * 1e-6
    assert abs(value - (answer + jd.SPRING_TORQUE * 1e-6)) <= 0.1 * jd.SPRING_TORQUE * 1e-6


def test_tilted_slider_accelerates_at_g_sin_theta(paths):
    """Semi-implicit Euler gives v = a t exactly for a constant force; the perpendicular term only acts across the axis.  The
    anchor hangs off the axis by the load across it times the regularisation, g cos(theta) * 1e-6 after the correction and
    g cos(theta) * (h^2 + 1e-6) before it."""
    value, answer = figure(paths, "incline")
    assert abs(value - answer) <= velocity_noise(600)
    off_axis, _ = figure(paths, "incline_perpendicular")
    assert 0.0 < off_axis <= jd.G * math.cos(jd.TILT) * (H20 * H20 + 1e-6)


def test_slide_limit_stops_the_slide(paths):
    """The stop is a spring of 1 / 1e-6 N/m (the regularisation): a body of 1 kg arriving at v sinks in by at most v / 1000 s.
    It arrives at sqrt(2 a stop) < 1.7 m/s."""
    value, answer = figure(paths, "incline_stop")
    arrival = math.sqrt(2 * jd.G * math.sin(jd.TILT) * jd.SLIDE_STOP)
    assert answer < value <= answer + arrival * 1e-3 + arrival * H20   # (+ one substep's travel: the stop is seen after integrate)
    free, free_answer = figure(paths, "incline_free")
    assert abs(free - free_answer) <= 0.5 * jd.G * math.sin(jd.TILT) * 0.5 * H20 * 1.001   # Euler's 1/2 a t h
    assert free > 1.9 * jd.SLIDE_STOP


def test_max_force_below_the_load_stalls_and_above_it_lifts(paths):
    """Clamped, the drive is a constant force: the load of 9.81 N falls against 5 N at (g - 5) exactly.  Unclamped it holds the
    speed but for the sag of the regularisation under the load, g * 1e-6 per substep: g * 1e-6 / h in speed."""
    value, answer = figure(paths, "lift_weak")
    assert abs(value - answer) <= velocity_noise(600)
    value, answer = figure(paths, "lift_strong")
    sag = jd.G * 1e-6 / H20
    assert abs(value - (answer - sag)) <= 1e-3 * sag + velocity_noise(600)
    assert value > 0.98 * answer


def test_hinge_limit_zero_makes_a_slider_prismatic(paths):
    """Spun at 5 rad/s, the slider turns by 5 h in its first substep before the limit 0/0 has acted once; it never gets further,
    while the control without the limit turns on (5 rad/s for 0.2 s)."""
    value, _ = figure(paths, "prismatic")
    assert 0.0 < value <= 5.0 * H20
    control, _ = figure(paths, "cylindrical")
    assert control > 0.99
    slid = jd.angle_and_offset(paths["prismatic"][-1], jd.scene("prismatic")[1][0])[1]
    assert abs(slid - 0.2) <= 1e-9                                      # the limit does not hold back the slide: 1 m/s for 0.2 s
