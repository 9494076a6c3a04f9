"""Known answers for the independent model of the overlap queries (tests/overlap_model.py)."""
import math

import numpy as np
import pytest

import overlap_model as om
import raycast_model as rm
from constraint_solver_amd import capi

IDENT = [1.0, 0.0, 0.0, 0.0]
CUBE = rm.box((-0.5, -0.5, -0.5), (0.5, 0.5, 0.5))                   # a unit cube about its centre


def cube_at(x, y=0.0, z=0.0, rotation=IDENT):
    return capi.overlap_queries([[x, y, z]], [rotation], 0)


def one_cube_scene(groups=None):
    return om.Scene([rm.rigid((0.0, 0.0, 0.0))], [0], [CUBE], groups)


@pytest.mark.parametrize("distance,hit", [(0.9, True), (1.0, False), (1.1, False)])
def test_two_unit_cubes_along_an_axis(distance, hit):
    offsets, hits = one_cube_scene().overlap(cube_at(distance))
    assert list(offsets) == [0, 1 if hit else 0]
    if hit:
        assert hits["body"][0] == 0 and hits["feature"][0] in (om.ob.FEATURE_FACE_A, om.ob.FEATURE_FACE_B)
        assert abs(hits["separation"][0] + 0.1) < 1e-15


def test_an_edge_against_an_edge_gives_the_edge_feature():
    # the body turned 45 degrees about z: its edge along z points at +x, at x = sqrt(1/2); the query cube turned 45 degrees about
    # y shows an edge along y towards -x.  The two edges cross at right angles and overlap by 0.05.
    half = math.pi / 8.0
    body = rm.rigid((0.0, 0.0, 0.0), (math.cos(half), 0.0, 0.0, math.sin(half)))
    scene = om.Scene([body], [0], [CUBE])
    q = cube_at(2.0 * math.sqrt(0.5) - 0.05, rotation=[math.cos(half), 0.0, math.sin(half), 0.0])
    offsets, hits = scene.overlap(q)
    assert list(offsets) == [0, 1] and hits["feature"][0] == om.ob.FEATURE_EDGES
    assert abs(hits["separation"][0] + 0.05) < 1e-12


def test_a_query_at_a_bodys_own_pose_hits_it_with_face_a():
    rot = np.array([0.9, 0.1, -0.3, 0.2])
    rot /= np.linalg.norm(rot)
    scene = om.Scene([rm.rigid((0.3, -0.2, 1.5), rot)], [0], [CUBE])
    offsets, hits = scene.overlap(capi.overlap_queries([[0.3, -0.2, 1.5]], [rot], 0))
    assert list(offsets) == [0, 1] and hits["feature"][0] == om.ob.FEATURE_FACE_A and hits["separation"][0] < -0.9


def test_ignore_and_mask_are_honoured():
    bodies = [rm.rigid((0.0, 0.0, 0.0)), rm.rigid((0.2, 0.0, 0.0)), rm.rigid((0.4, 0.0, 0.0))]
    scene = om.Scene(bodies, [0, 0, 0], [CUBE], groups=[1, 2, 0])
    q = capi.overlap_queries([[0.1, 0.0, 0.0]], [IDENT], 0)
    assert list(scene.overlap(q)[1]["body"]) == [0, 1, 2]
    q["ignore_body"] = 1
    assert list(scene.overlap(q)[1]["body"]) == [0, 2]
    q["ignore_body"] = capi.NO_HIT
    for mask, want in ((1, [0]), (2, [1]), (3, [0, 1]), (4, []), (0, [])):
        q["mask"] = mask
        assert list(scene.overlap(q, masked=True)[1]["body"]) == want
        assert list(scene.overlap(q, masked=False)[1]["body"]) == [0, 1, 2]          # without the flag the mask is not read
    unfiltered = om.Scene(bodies, [0, 0, 0], [CUBE])                                  # bodies without filters: group ~0
    q["mask"] = 4
    assert list(unfiltered.overlap(q, masked=True)[1]["body"]) == [0, 1, 2]


def test_frames_that_are_not_finite_report_nothing():
    scene = one_cube_scene()
    for bad in (np.nan, np.inf, -np.inf):
        q = cube_at(0.0)
        q["position"][0, 1] = bad
        assert list(scene.overlap(q)[0]) == [0, 0]
        q = cube_at(0.0)
        q["rotation"][0, 2] = bad
        assert list(scene.overlap(q)[0]) == [0, 0]
    nan_body = om.Scene([rm.rigid((np.nan, 0.0, 0.0)), rm.rigid((0.0, 0.0, 0.0))], [0, 0], [CUBE])
    assert list(nan_body.overlap(cube_at(0.0))[1]["body"]) == [1]
    assert list(one_cube_scene().overlap(capi.overlap_queries([[0.0, 0.0, 0.0]], [IDENT], 3))[0]) == [0, 0]   # no such shape
