"""The three joint setters (xpbd_world_set_joints, _set_joint_limits, _set_joint_drives) stage the part of the joint tables
they replace and move it in.  So the tables depend on the settings in force and not on the calls that led there: a world driven
through a sequence of setter calls steps bit for bit like a fresh world given the final settings once.  The 130-body box scene
of population_common.py reaches every branch of the three table builders: three waves, a pair joined three times, a joint given
with body_a > body_b, hinges and sliders, limits and drives out of joint order, and slide, hinge and drive entries on one joint.
EXTENSION: parity unpinned."""
import numpy as np
import pytest

import population_common as pc
from body_edit_common import N, scene, world
from constraint_solver_amd import capi
from population_common import REMOVED, apply_settings, expected_map, newcomers, reindex_settings, same_runs, settings_for

pytestmark = pytest.mark.gpu

BOXES = capi.SCENE_BOXES_DROP
FRAMES = 2
S = settings_for()


def without(s, *keys):
    return dict(s, **{k: s[k][:0] for k in keys})


def others(w, s):
    """What apply_settings sets after the joints."""
    w.set_collision_filters(s["filters"], capi.FILTER_JOINTED)
    w.set_materials(s["mu"], 0.6)
    w.set_restitution(s["e"], 0.5, 0.1)
    w.set_contact_report(True)


def fresh_run(s, bodies=None, sid=None):
    """A fresh world given the settings `s` once."""
    if bodies is None:
        bodies, sid = scene(BOXES)
    with world(BOXES, bodies, sid) as w:
        apply_settings(w, s)
        return pc.run(w, FRAMES, True)


def driven_run(calls, s=S):
    """A world driven through `calls` (each takes the world), then given the settings of `s` that are not the joints'."""
    bodies, sid = scene(BOXES)
    with world(BOXES, bodies, sid) as w:
        for call in calls:
            call(w)
        others(w, s)
        return pc.run(w, FRAMES, True)


@pytest.fixture(scope="module")
def full():
    return fresh_run(S)


def joints(s=S):
    return lambda w: w.set_joints(s["joints"])


def lims(s=S):
    return lambda w: w.set_joint_limits(s["lims"])


def drives(s=S):
    return lambda w: w.set_joint_drives(s["drives"])


# ---- 1. limits and drives do not clear each other ---------------------------------------------------------------------------------
def test_drives_then_limits_equals_limits_then_drives(full):
    assert same_runs(driven_run([joints(), drives(), lims()]), full)


# ---- 2. set, then cleared with an empty array, equals never set -------------------------------------------------------------------
@pytest.mark.parametrize("what", ["drives", "lims"])
def test_cleared_equals_never_set(full, what):
    none = without(S, what)
    first, second = (drives, lims) if what == "drives" else (lims, drives)
    got = driven_run([joints(), first(), first(none), second()])
    assert same_runs(got, fresh_run(none))
    assert not same_runs(got, full)                                      # (what was cleared had changed the run)


# ---- 3. SLIDE limits leave and come back: the extras shrink and grow --------------------------------------------------------------
def test_slide_limits_replaced_by_the_angular_ones_and_back(full):
    angular = dict(S, lims=S["lims"][S["lims"]["kind"] != capi.LIMIT_SLIDE])
    assert 0 < len(angular["lims"]) < len(S["lims"])
    to_angular = [joints(), lims(), drives(), lims(angular)]
    got = driven_run(to_angular)
    assert same_runs(got, fresh_run(angular)) and not same_runs(got, full)   # (the SLIDE limits bind within the two frames)
    assert same_runs(driven_run(to_angular + [lims()]), full)


# ---- 4. new joints drop limits and drives -----------------------------------------------------------------------------------------
def test_new_joints_drop_limits_and_drives(full):
    half = without(dict(S, joints=S["joints"][:len(S["joints"]) // 2]), "lims", "drives")
    kinds = set(half["joints"]["kind"])
    assert {capi.JOINT_HINGE, capi.JOINT_SLIDER, capi.JOINT_DISTANCE} <= kinds
    to_half = [joints(), lims(), drives(), joints(half)]
    got = driven_run(to_half)
    assert same_runs(got, fresh_run(half)) and not same_runs(got, full)
    none = without(S, "joints", "lims", "drives")
    assert same_runs(driven_run(to_half + [joints(none)]), fresh_run(none))


# ---- 5. a setter on top of a committed population change --------------------------------------------------------------------------
def test_drives_set_after_a_population_change_see_the_reindexed_joints():
    bodies, sid = scene(BOXES)
    added, added_sid = newcomers(BOXES, 3)
    want_map, keep = expected_map(N, REMOVED)
    final = reindex_settings(S, want_map, len(added))
    assert 0 < len(final["drives"]) and 0 < len(final["joints"]) < len(S["joints"])
    final["drives"]["target"] = -final["drives"]["target"]
    with world(BOXES, bodies, sid) as w:
        apply_settings(w, S)
        w.remove_bodies(REMOVED)
        w.add_bodies(added, added_sid)
        w.set_joint_drives(final["drives"])
        changed = w.download()
        got = pc.run(w, FRAMES, True)
    assert same_runs(got, fresh_run(final, changed, np.concatenate([sid[keep], added_sid])))


# ---- 6. a rejected call changes nothing -------------------------------------------------------------------------------------------
def rejected(w):
    """An XPBD_E_INVALID call of each setter: a joint naming body n, a limit of unknown kind, a drive on joint len(joints)."""
    bad_joints = S["joints"].copy()
    bad_joints["body_b"][0] = w.n
    bad_lims = S["lims"][:2].copy()
    bad_lims["kind"][1] = 99
    bad_drives = S["drives"][:2].copy()
    bad_drives["joint"][1] = len(S["joints"])
    for call, value in [(w.set_joints, bad_joints), (w.set_joint_limits, bad_lims), (w.set_joint_drives, bad_drives)]:
        with pytest.raises(capi.XpbdError) as e:
            call(value)
        assert e.value.code == capi.E_INVALID


def test_rejected_calls_between_the_setters_change_nothing(full):
    assert same_runs(driven_run([joints(), rejected, drives(), rejected, lims(), rejected]), full)
