"""The shape tables of a world have one owner and one staged install (ShapeTables, csrc/xpbd_world.hpp;
csrc/xpbd_world_shapes.cpp): a refused setter changes nothing, tables replace each other whole whether they grow or shrink, a
vertex-only set drops the topology and a polytope set brings it back, and the multi-GPU world -- which compiles the tables once
for all its shards -- plans and steps as it did when every shard compiled its own (a recorded run: golden/shape_tables_multi.json).
Three to six bodies in touching poses, four substeps, XPBD_MODE_CONTACTS."""
import numpy as np
import pytest

from constraint_solver_amd import capi
from golden_util import bits_equal, load, unhex

pytestmark = pytest.mark.gpu

DT, SUBSTEPS = 1.0 / 60.0, 4
PLAN_KEYS = ("plans", "rollbacks", "migrated", "owned_min", "owned_max", "steps", "full_plans", "light_plans")   # (the others are times)


def tables():
    """A: cube, tetrahedron.  B: one more shape, more vertices, and both size classes (the icosahedron has 12 vertices)."""
    b = capi.scene_polytopes(capi.SCENE_MIXED_DROP)
    return b[:2], b


def scene(sid, positions):
    """Bodies of the mixed scene's shapes `sid` (its body k has shape k mod 3) at rest at `positions`, unrotated."""
    rows, shape = capi.scene_generate(capi.SCENE_MIXED_DROP, 1, 6)
    assert list(shape) == [0, 1, 2, 0, 1, 2]
    bodies = np.stack([rows[s] for s in sid])
    bodies[:, 22:28] = 0.0
    bodies[:, 31:34] = positions
    bodies[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    return bodies, np.array(sid, dtype=np.uint32)


def scene_a():
    """cube, cube, tetrahedron: the cubes side by side 1 cm into each other, the tetrahedron 1 cm into the first one's top"""
    return scene([0, 0, 1], [[0.0, 0.0, 0.0], [0.99, 0.0, 0.0], [0.3, 0.3, 0.99]])


def scene_b():
    """cube, tetrahedron, icosahedron, cube: a shape of every row of table B, each touching the first cube"""
    return scene([0, 1, 2, 0], [[0.0, 0.0, 0.0], [0.99, 0.2, 0.0], [0.5, 0.5, 1.49], [0.0, 0.99, 0.0]])


def world(polys, bodies, sid):
    w = capi.World(mode=capi.MODE_CONTACTS)
    w.set_polytopes(polys)
    w.upload(bodies, sid)
    return w


def steps(w, frames):
    for _ in range(frames):
        w.step(DT, SUBSTEPS)
    return w.download()


def broken(polys):
    """`polys` with a face of shape 0 naming a vertex the shape does not have."""
    bad = [dict(p) for p in polys]
    bad[0]["face_indices"] = bad[0]["face_indices"].copy()
    bad[0]["face_indices"][1] = 99
    return bad


def test_a_refused_call_changes_nothing():
    a, _ = tables()
    bodies, sid = scene_a()
    with world(a, bodies, sid) as w, world(a, bodies, sid) as twin:
        assert bits_equal(steps(w, 2), steps(twin, 2)) and w.contact_stats()[1] > 0
        with pytest.raises(capi.XpbdError) as e:
            w.set_polytopes(broken(a))
        assert e.value.code == capi.E_INVALID and "xpbd_world_set_polytopes: shape 0 face vertex out of range" in str(e.value)
        with pytest.raises(capi.XpbdError) as e:
            w.set_shapes(a[0]["vertices"], [0, 8])                      # one shape, but body 2 has shape id 1
        assert e.value.code == capi.E_INVALID and "xpbd_world_set_shapes: 1 shapes, but the uploaded bodies use shape id 1" in str(e.value)
        got, want = steps(w, 2), steps(twin, 2)
        assert bits_equal(got, want) and not np.isnan(got).any()


@pytest.mark.parametrize("order", ["A then B", "B then A"])
def test_replacing_works_both_ways(order):
    """The world had one table (and bodies, and a frame); given the other, a fresh upload and a step it is a fresh world given the
    other alone: the tables grow (2 -> 3 shapes, 12 -> 24 vertices, one size class -> two) and shrink."""
    a, b = tables()
    first, then = ((a, scene_a()), (b, scene_b())) if order == "A then B" else ((b, scene_b()), (a, scene_a()))
    with world(first[0], *first[1]) as w, world(then[0], *then[1]) as fresh:
        steps(w, 1)
        w.upload(*scene_a())                                           # (bodies whose shapes both tables have: a shrinking table is
        w.set_polytopes(then[0])                                       # refused while a resident body uses a shape it drops)
        w.upload(*then[1])
        got, want = steps(w, 2), steps(fresh, 2)
        assert bits_equal(got, want) and not np.isnan(got).any()
        assert fresh.contact_stats()[1] > 0


def test_topology_can_be_dropped_and_restored():
    a, _ = tables()
    bodies, sid = scene_a()
    verts = np.concatenate([p["vertices"] for p in a])
    offsets = np.cumsum([0] + [len(p["vertices"]) for p in a])
    down = capi.rays([[0.5, 0.5, 5.0]], [[0.0, 0.0, -1.0]])
    with world(a, bodies, sid) as w, world(a, bodies, sid) as twin:
        assert bits_equal(steps(w, 1), steps(twin, 1))
        assert w.raycast(down)["body"][0] != capi.NO_HIT
        w.set_shapes(verts, offsets)                                    # vertices only: the polytope topology is gone
        with pytest.raises(capi.XpbdError) as e:
            w.step(DT, SUBSTEPS)
        assert e.value.code == capi.E_INVALID and "XPBD_MODE_CONTACTS needs xpbd_world_set_polytopes" in str(e.value)
        with pytest.raises(capi.XpbdError) as e:
            w.raycast(down)
        assert e.value.code == capi.E_INVALID
        assert "xpbd_world_raycast: call xpbd_world_set_polytopes (set_shapes gives vertices only) first" in str(e.value)
        w.set_polytopes(a)
        got, want = steps(w, 2), steps(twin, 2)
        assert bits_equal(got, want) and not np.isnan(got).any()


def multi_scene():
    """Six bodies of the three shapes in a row along x, neighbours about 1 cm into each other where they meet."""
    return scene([0, 1, 2, 0, 1, 2], [[0.0, 0.0, 0.0], [0.99, 0.0, 0.0], [1.98, 0.5, 0.5], [2.47, 0.0, 0.0], [3.46, 0.0, 0.0], [4.45, 0.5, 0.5]])


def multi_run(mw):
    bodies, sid = multi_scene()
    mw.upload(bodies, sid, 0, len(bodies))
    for _ in range(2):
        mw.step(DT, SUBSTEPS)
    stats = mw.plan_stats()
    return {k: stats[k] for k in PLAN_KEYS}, mw.download(), mw.contact_stats()


def multi_world():
    return capi.MultiWorld(2, devices=[0, 0], transport=capi.TRANSPORT_LOCAL, halo_margin=0.75, auto_replan=True)


def test_the_multi_gpu_world_plans_and_steps_as_recorded():
    """Two ranks on one device.  The record was made before the multi-GPU world compiled the tables once: the planner's radii and
    centroids then came from a loop of its own, and every shard compiled the tables again."""
    golden = load("shape_tables_multi.json")
    with multi_world() as mw:
        mw.set_polytopes(tables()[1])
        stats, got, contacts = multi_run(mw)
    assert stats == golden["plan_stats"]
    assert contacts[1] > 0 and list(contacts) == golden["contact_stats"]
    assert bits_equal(got, unhex(golden["bodies"], (6, capi.RIGID_DOUBLES)))


def test_a_refused_multi_gpu_set_leaves_upload_refused():
    bodies, sid = multi_scene()
    _, b = tables()
    with multi_world() as mw:
        for _ in ("on a fresh world", "after a valid set"):
            with pytest.raises(capi.XpbdError) as e:
                mw.set_polytopes(broken(b))
            assert e.value.code == capi.E_INVALID and "xpbd_world_set_polytopes: shape 0 face vertex out of range" in str(e.value)
            with pytest.raises(capi.XpbdError) as e:
                mw.upload(bodies, sid, 0, len(bodies))
            assert e.value.code == capi.E_INVALID and "xpbd_multi_world_upload: call xpbd_multi_world_set_polytopes first" in str(e.value)
            mw.set_polytopes(b)
        stats, got, _ = multi_run(mw)                                   # ... and the valid set after it stands
    golden = load("shape_tables_multi.json")
    assert stats == golden["plan_stats"] and bits_equal(got, unhex(golden["bodies"], (6, capi.RIGID_DOUBLES)))
