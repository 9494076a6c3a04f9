"""The terrain model (tests/terrain_model.py) on the CPU: first that it is a faithful restatement -- on a flat field it equals
material_model.Model bit for bit --, then the lookup on a tilted plane, and a box on a real slope under plain gravity, which
must stick and slide by the project's own thresholds before the device is held to them (tests/test_gpu_terrain.py)."""
import math
import sys

import numpy as np
import pytest

import material_model as mm
import oracle_binding as ob
import terrain_model as tm
from constraint_solver_amd import capi
from golden_util import bits_equal
from halo_common import POLY_NAMES, pile

DT = 1.0 / 60.0
G = 9.81
EPS = sys.float_info.epsilon


@pytest.mark.parametrize("speed", [0.0, 3.0])
def test_flat_field_is_the_plane_bit_for_bit(speed):
    """x - s * n reproduces {x.x, x.y, 0.0} and the contact test is !(x.z >= 0) when n = (-0, -0, 1) and d = 0."""
    kind, n = capi.SCENE_BOXES_DROP, 24
    bodies, sid = pile(capi, kind, n, 2, 2.5, 2.0)
    bodies[:, 31:33] += 9.0                                     # the pile bursts: boxes travel metres sideways in these 4 frames
    bodies[:, 33] -= 0.6                                        # ... and the lowest start in the ground: contacts from frame 0
    polys = ob.polytopes_array(POLY_NAMES[kind])
    mu = np.random.default_rng(4).choice([0.0, 0.2, 0.5, 1.0], n)
    field = tm.Terrain(tm.flat_field(40, 30), (-3.1, -2.3), (0.7, 0.9))         # covers [-3.1, 24.2) x [-2.3, 23.8)
    plane = mm.Model(bodies, sid, polys, mu, 0.4, max_depenetration_speed=speed)
    terrain = tm.Model(bodies, sid, polys, field, mu=mu, ground_mu=0.4, max_depenetration_speed=speed)
    contacts = 0
    for _ in range(4):
        plane.ground_trace, terrain.ground_trace = [], []
        want, got = plane.step(DT, 6), terrain.step(DT, 6)
        assert got[:, 31:33].min() > 0.0 and got[:, 31:33].max() < 21.0           # (a check of the scene: nobody left the field)
        assert bits_equal(got, want)
        assert len(terrain.ground_trace) == len(plane.ground_trace)
        contacts += len(plane.ground_trace)
    assert contacts > 50 and not np.isnan(want).any()
    assert any(terrain.masks)


def test_every_lookup_on_a_tilted_plane_returns_the_same_plane():
    """h = 0.25 x + 0.1 y sampled where every height is exact (x a multiple of 0.5, y of 2.5), so both slopes are the same
    two doubles in every triangle and n has the same bits everywhere.  d = dot(n, corner) is rounded per cell: three products
    and two sums, each within half an ulp of a term no larger than M = |n.x cx| + |n.y cy| + |n.z h|, so two cells' d differ
    by less than 5 eps M; 8 eps M is asserted."""
    origin, cell = (-3.0, -5.0), (0.5, 2.5)
    x = origin[0] + np.arange(14) * cell[0]
    y = origin[1] + np.arange(6) * cell[1]
    heights = 0.25 * x[None, :] + (y / 10.0)[:, None]
    field = tm.Terrain(heights, origin, cell)
    rng = np.random.default_rng(1)
    first = None
    for _ in range(400):
        p = (rng.uniform(-3.0, 3.5), rng.uniform(-5.0, 7.5), rng.uniform(-1.0, 1.0))
        plane = field.plane(p)
        assert plane is not None
        n, d = plane
        first = first or plane
        assert n == first[0]
        bound = 8.0 * EPS * (abs(n[0]) * 3.5 + abs(n[1]) * 7.5 + abs(n[2]) * 2.0)
        assert abs(d - first[1]) <= bound
        h, normal = field.sample(p[0], p[1])
        assert normal == n and abs(h - (0.25 * p[0] + 0.1 * p[1])) < 1e-14
    assert abs(first[0][0] / first[0][2] + 0.25) < 1e-15 and abs(first[0][1] / first[0][2] + 0.1) < 1e-15
    assert field.plane((3.5, 0.0, 0.0)) is None and field.plane((0.0, 7.5, 0.0)) is None          # the far edges are outside
    assert field.plane((math.nan, 0.0, 0.0)) is None and field.plane((-3.0000001, 0.0, 0.0)) is None
    assert field.plane((-3.0, -5.0, 0.0)) is not None


def slide(tan_theta, mu, frames, substeps=20):
    """Distance along the slope, downhill, that a box lying on the tilted-plane field h = tan_theta * x has covered."""
    bodies, sid, theta, downhill = tm.box_on_slope(capi, tan_theta)
    origin, cell = (-12.0, -3.0), (1.0, 1.0)
    field = tm.Terrain(tm.tilted_field(17, 8, origin, cell, tan_theta), origin, cell)
    model = tm.Model(bodies, sid, ob.polytopes_array(POLY_NAMES[capi.SCENE_BOXES]), field, mu=[mu], ground_mu=mm.INF)
    start = model.bodies[0, 31:34].copy()
    for _ in range(frames):
        model.step(DT, substeps)
    assert any(model.masks)
    return float(np.dot(model.bodies[0, 31:34] - start, downhill)), theta


def test_box_on_a_real_slope_sticks_below_and_slides_above_the_friction_angle():
    """The experiment of test_material_model.py's slope tests with the slope in the ground instead of in gravity."""
    d, theta = slide(0.25, 0.5, 60)
    free = 0.5 * G * math.sin(theta)
    print("terrain, gentle slope: moved %.3e m of %.3f m (%.2f %%)" % (d, free, 100.0 * d / free))
    assert abs(d) < mm.STICKS * free
    d, theta = slide(1.0, 0.5, 60)
    free = 0.5 * G * math.sin(theta)
    print("terrain, steep slope: moved %.4f m of %.3f m" % (d, free))
    assert mm.SLIDES * free < d < (1.0 - mm.SLIDES) * free
