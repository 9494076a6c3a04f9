"""The ray-cast model (tests/raycast_model.py) against answers worked out by hand: boxes, a rotated box, a tetrahedron and an
icosahedron with offset centres of mass; rays from inside, parallel to a face, ending exactly at a surface; ties; invalid rays."""
import math

import numpy as np
import pytest

import raycast_model as rm

RAY = np.dtype([("origin", "<f8", (3,)), ("direction", "<f8", (3,)), ("max_distance", "<f8"), ("ignore_body", "<u4"),
                ("reserved", "<u4")])


def rays(origins, directions, max_distance=np.inf, ignore=rm.NO_HIT):
    o, d = np.atleast_2d(np.asarray(origins, float)), np.atleast_2d(np.asarray(directions, float))
    out = np.zeros(max(len(o), len(d)), dtype=RAY)
    out["origin"], out["direction"], out["max_distance"], out["ignore_body"] = o, d, max_distance, ignore
    return out


def cast(bodies, sid, polys, r):
    hits, _ = rm.raycast(np.atleast_2d(bodies), np.asarray(sid), polys, r)
    return hits


def test_axis_aligned_and_oblique_rays_at_a_unit_box_with_offset_centre_of_mass():
    body = rm.rigid((2.0, 0.0, 0.0), com=(0.5, 0.5, 0.5))               # identity rotation: the box spans [2, 3] x [0, 1]^2
    h = cast(body, [0], [rm.box()], rays([[0.0, 0.5, 0.5], [2.5, 0.5, 5.0], [0.0, 0.0, 0.0]],
                                         [[1.0, 0.0, 0.0], [0.0, 0.0, -2.0], [2.5, 0.5, 0.5]]))
    assert list(h["body"]) == [0, 0, 0]
    assert h["distance"][0] == 2.0 and h["face"][0] == 4                 # enters through -x
    np.testing.assert_array_equal(h["normal"][0], [-1.0, 0.0, 0.0])
    np.testing.assert_array_equal(h["point"][0], [2.0, 0.5, 0.5])
    assert h["distance"][1] == 2.0 and h["face"][1] == 1                 # |direction| = 2: t in units of it
    np.testing.assert_array_equal(h["normal"][1], [0.0, 0.0, 1.0])
    assert h["distance"][2] == pytest.approx(0.8) and h["face"][2] == 4  # (2, 0.4, 0.4) on the -x face


def test_box_rotated_45_degrees_about_z():
    c, s = math.cos(math.pi / 8), math.sin(math.pi / 8)
    body = rm.rigid((-0.5, -0.5, -0.5), rotation=(c, 0.0, 0.0, s), com=(0.5, 0.5, 0.5))   # centred at the origin
    h = cast(body, [0], [rm.box()], rays([[-5.0, 0.0, 0.0]], [[1.0, 0.0, 0.0]]))
    assert h["body"][0] == 0
    assert h["distance"][0] == pytest.approx(5.0 - math.sqrt(0.5), abs=1e-12)   # the vertex at x = -sqrt(2)/2
    h = cast(body, [0], [rm.box()], rays([[-5.0, 0.2, 0.0]], [[1.0, 0.0, 0.0]]))
    assert h["distance"][0] == pytest.approx(5.0 - (math.sqrt(0.5) - 0.2), abs=1e-12)
    n = h["normal"][0]
    assert n[2] == pytest.approx(0.0, abs=1e-15) and n[0] == pytest.approx(-math.sqrt(0.5)) and n[1] == pytest.approx(math.sqrt(0.5))


def test_tetrahedron_and_icosahedron():
    polys = [rm.tetrahedron(), rm.icosahedron(0.5)]
    bodies = np.stack([rm.rigid((0.0, 0.0, 0.0), com=(0.25, 0.25, 0.25)), rm.rigid((5.0, 0.0, 0.0), com=(0.1, -0.2, 0.3))])
    h = cast(bodies, [0, 1], polys, rays([[1.0, 1.0, 1.0], [5.0, 0.0, 4.0]], [[-1.0, -1.0, -1.0], [0.0, 0.0, -1.0]]))
    assert list(h["body"]) == [0, 1]
    assert h["distance"][0] == pytest.approx(2.0 / 3.0)                  # plane x + y + z = 1
    np.testing.assert_allclose(h["normal"][0], np.ones(3) / math.sqrt(3.0), rtol=1e-15)
    # icosahedron of circumradius 0.5 about the origin: the ray down the z axis meets it between inradius and circumradius
    inradius = 0.5 * math.sqrt(3.0) / 12.0 * (3.0 + math.sqrt(5.0)) / (math.sqrt(10.0 + 2.0 * math.sqrt(5.0)) / 4.0)
    assert 4.0 - 0.5 <= h["distance"][1] <= 4.0 - inradius + 1e-12


def test_ray_from_inside_hits_at_zero_with_no_face():
    h = cast(rm.rigid((0.0, 0.0, 0.0)), [0], [rm.box()], rays([[0.5, 0.5, 0.5]], [[0.0, 1.0, 0.0]]))
    assert h["body"][0] == 0 and h["distance"][0] == 0.0 and h["face"][0] == rm.RAY_INSIDE
    np.testing.assert_array_equal(h["normal"][0], [0.0, 0.0, 0.0])
    np.testing.assert_array_equal(h["point"][0], [0.5, 0.5, 0.5])


def test_ray_parallel_to_a_face_inside_and_outside_its_slab():
    body, poly = rm.rigid((0.0, 0.0, 0.0)), [rm.box()]
    h = cast(body, [0], poly, rays([[-1.0, 0.5, 0.5], [-1.0, 1.5, 0.5]], [[1.0, 0.0, 0.0], [1.0, 0.0, 0.0]]))
    assert h["body"][0] == 0 and h["distance"][0] == 1.0
    assert h["body"][1] == rm.NO_HIT and h["distance"][1] == np.inf


def test_hit_exactly_at_max_distance_and_one_ulp_short():
    body, poly = rm.rigid((0.0, 0.0, 0.0)), [rm.box()]
    h = cast(body, [0], poly, rays([[-1.0, 0.5, 0.5]] * 2, [[1.0, 0.0, 0.0]] * 2, max_distance=np.array([1.0, np.nextafter(1.0, 0.0)])))
    assert h["body"][0] == 0 and h["distance"][0] == 1.0
    assert h["body"][1] == rm.NO_HIT


def test_equal_t_goes_to_the_smaller_index_and_ignore_body():
    bodies = np.stack([rm.rigid((0.0, 0.0, 0.0)), rm.rigid((0.0, 1.0, 0.0)), rm.rigid((0.0, -1.0, 0.0))])
    r = rays([[-1.0, 1.0, 0.5]], [[1.0, 0.0, 0.0]])                      # along the face shared by bodies 0 and 1
    h = cast(bodies, [0, 0, 0], [rm.box()], r)
    assert h["body"][0] == 0 and h["distance"][0] == 1.0
    r["ignore_body"] = 0
    h = cast(bodies, [0, 0, 0], [rm.box()], r)
    assert h["body"][0] == 1 and h["distance"][0] == 1.0


def test_invalid_rays_hit_nothing():
    body = rm.rigid((0.0, 0.0, 0.0))
    bad = rays([[np.nan, 0.5, 0.5], [-1.0, 0.5, 0.5], [-1.0, 0.5, 0.5], [-1.0, 0.5, 0.5], [-np.inf, 0.5, 0.5], [-1.0, 0.5, 0.5]],
               [[1.0, 0.0, 0.0], [0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 0.0, 0.0], [np.inf, 0.0, 0.0]],
               max_distance=np.array([np.inf, np.inf, -1.0, np.nan, np.inf, np.inf]))
    h = cast(body, [0], [rm.box()], bad)
    assert (h["body"] == rm.NO_HIT).all() and (h["distance"] == np.inf).all()


def test_planes_point_away_from_the_centroid():
    for poly in (rm.box(), rm.tetrahedron(0.5), rm.icosahedron(0.5)):
        pl = rm.polytope_planes(poly)
        d = pl[:, :3] @ poly["centroid"] - pl[:, 3]
        assert (d < 0).all()
        np.testing.assert_allclose(np.linalg.norm(pl[:, :3], axis=1), 1.0, rtol=1e-15)
