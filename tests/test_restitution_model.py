"""The model of restitution (tests/restitution_model.py) on the CPU: first that with every coefficient 0 it is the oracle's
contact pipeline bit for bit, then what the velocity pass does in it -- a dropped box bounces by its coefficient, two boxes
that meet head-on separate with their momentum kept, a contact takes the larger coefficient of its two sides, and a box at rest
stays at rest under a bounce threshold.  The bounds and the measurements behind them are in restitution_model.py."""
import numpy as np
import pytest

import oracle_binding as ob
import restitution_model as rm
from constraint_solver_amd import capi
from golden_util import bits_equal
from halo_common import POLY_NAMES, pile

DT = 1.0 / 60.0
BOXES = ob.polytopes_array(POLY_NAMES[capi.SCENE_BOXES])
ES = np.array([0.0, 0.3, 0.8, 1.0])


# ---- faithful: all coefficients 0 is the oracle, bit for bit ----------------------------------------------------------------
@pytest.mark.parametrize("speed", [0.0, 3.0])
@pytest.mark.parametrize("kind,n,seed", [(capi.SCENE_BOXES_DROP, 40, 3), (capi.SCENE_MIXED_DROP, 48, 5)])
def test_model_without_restitution_is_the_oracle(kind, n, seed, speed):
    """The scenes of test_material_model.py."""
    bodies, sid = pile(capi, kind, n, seed, 3.0, 2.5)
    polys = ob.polytopes_array(POLY_NAMES[kind])
    model = rm.Model(bodies, sid, polys, [0.0] * n, 0.0, 0.0, pad=0.02, max_depenetration_speed=speed)
    want, stats = bodies, ob.ContactStats()
    for _ in range(12):
        got = model.step(DT, 6)
        want = ob.contacts_step_joints(want, sid, polys, np.zeros(0, dtype=capi.JOINT_DTYPE), DT, 6, 0.02, stats=stats,
                                       max_depenetration_speed=speed)
        assert bits_equal(got, want)
    assert not np.isnan(want).any() and stats.n_points > 50
    assert model.pair_entries == 0 and model.ground_entries == 0


def test_the_pass_fires_on_these_scenes_and_changes_the_result():
    kind, n = capi.SCENE_MIXED_DROP, 48
    bodies, sid = pile(capi, kind, n, 5, 3.0, 2.5)
    polys = ob.polytopes_array(POLY_NAMES[kind])
    plain = rm.Model(bodies, sid, polys)
    bouncy = rm.Model(bodies, sid, polys, ES[np.random.default_rng(5).integers(0, 4, n)], 0.5)
    for _ in range(6):
        a, b = plain.step(DT, 6), bouncy.step(DT, 6)
    assert bouncy.pair_entries > 50 and bouncy.pair_impulses > 50 and bouncy.ground_entries > 10
    assert not np.isnan(b).any() and not bits_equal(a, b)
    assert bits_equal(a[:, 0:22], b[:, 0:22])                       # mass properties and forces are nobody's to write


# ---- a dropped box ------------------------------------------------------------------------------------------------------
def drop(e, ground_e=0.0, frames=110):
    bodies, sid = rm.dropped_box(capi, rm.DROP_HEIGHT)
    model = rm.Model(bodies, sid, BOXES, [e], ground_e)
    z, vz = [], []
    for _ in range(frames):
        model.step(DT, 20)
        z.append(float(model.bodies[0, 33]))
        vz.append(float(model.bodies[0, 24]))
    return z, vz, model


@pytest.mark.parametrize("e", [0.5, 0.8])
def test_dropped_box_bounces_by_its_coefficient(e):
    z, vz, model = drop(e)
    k = rm.bounce_frame(vz)
    ratio, apex = -vz[k] / vz[k - 1], rm.apex_after(z, k)
    print("drop e %.1f: frame %d, %.4f -> %.4f m/s, ratio %.4f; apex %.4f m of %.4f m" % (e, k, vz[k - 1], vz[k], ratio, apex,
                                                                                          e * e * rm.DROP_HEIGHT))
    assert model.ground_entries > 0 and model.pair_entries == 0
    assert abs(ratio - e) < rm.DROP_RATIO_BOUND
    assert abs(apex / (e * e * rm.DROP_HEIGHT) - 1.0) < rm.DROP_APEX_BOUND


def test_contact_takes_the_larger_coefficient():
    """Body 0.2 on a ground of 0.9 is a contact of 0.9: the same bits as 0.9 on 0.9 and as 0.9 on 0, and not those of 0.2."""
    want = drop(0.9, 0.9, 60)[2].bodies
    assert bits_equal(drop(0.2, 0.9, 60)[2].bodies, want)
    assert bits_equal(drop(0.9, 0.0, 60)[2].bodies, want)
    z, vz, model = drop(0.2, 0.0, 60)
    assert not bits_equal(model.bodies, want)
    k = rm.bounce_frame(vz)
    assert abs(-vz[k] / vz[k - 1] - 0.2) < rm.DROP_RATIO_BOUND


def test_box_at_rest_under_a_bounce_threshold_stays_at_rest_to_the_bit():
    """A resting box falls g h = 8.2 mm/s per substep before the ground stops it; a threshold of 1 m/s is far above that."""
    bodies, sid = rm.dropped_box(capi, 0.0)
    still, held, free = (rm.Model(bodies, sid, BOXES, [e], e, threshold) for e, threshold in ((0.0, 0.0), (0.8, 1.0), (0.8, 0.0)))
    for _ in range(30):
        a, b, c = still.step(DT, 20), held.step(DT, 20), free.step(DT, 20)
        assert bits_equal(a, b)
    assert held.ground_entries == 0
    assert free.ground_entries > 0 and not bits_equal(a, c)        # without the threshold the resting contact does bounce


# ---- two boxes head-on ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("e", [1.0, 0.5])
def test_boxes_head_on_leave_at_e_times_the_closing_speed_and_keep_their_momentum(e):
    bodies, sid = rm.head_on_boxes(capi, 1.0)
    model = rm.Model(bodies, sid, BOXES, [e, e])
    for _ in range(40):
        got = model.step(DT, 20)
    ratio = (got[1, 22] - got[0, 22]) / 2.0
    print("head-on e %.1f: velocities %.6f, %.6f m/s; relative speed after / before %.4f; momentum %.3e" % (e, got[0, 22], got[1, 22], ratio,
                                                                                                          got[0, 22] + got[1, 22]))
    assert model.pair_entries > 0 and model.ground_entries == 0
    assert got[0, 22] < 0.0 < got[1, 22]                                                    # they separate
    assert abs(got[0, 22] + got[1, 22]) < rm.HEAD_ON_MOMENTUM_BOUND                          # equal masses: momentum kept
    assert np.abs(got[:, 23:28]).max() < rm.HEAD_ON_SPIN_BOUND                              # nothing sideways, no spin
    assert abs(ratio - e) < rm.HEAD_ON_BOUND[e]                                          # e = 1: velocities exchanged; 0.5: halved
