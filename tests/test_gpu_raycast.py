"""Batched ray casts (xpbd_world_raycast*, xpbd_multi_world_raycast; EXTENSION) on the MI355X:
  * the grid path equals the brute-force path bit for bit in every field of every hit (piles of 262 144 boxes and 65 536
    mixed polyhedra, a sparse world on the hashed grid; random, outside, camera-fan, inside, axis-aligned, cell-face and
    ignore_body rays);
  * the device equals the independent model (tests/raycast_model.py) after stepping in every mode;
  * a ray cast has no side effect on stepping; the device variant equals the host variant; the sharded world equals the
    single one; argument errors."""
import numpy as np
import pytest

import raycast_model as rm
from constraint_solver_amd import capi

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
BRUTE = capi.RAYCAST_BRUTE_FORCE


def same_bits(a, b):
    return a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def stepped(bodies, sid, kind, frames, substeps=20, mode=capi.MODE_CONTACTS):
    w = capi.World(mode=mode)
    w.set_polytopes(capi.scene_polytopes(kind))
    w.upload(bodies, sid)
    for _ in range(frames):
        w.step(DT, substeps)
    return w


def cell_edge(kind, sid):
    """The query grid's cell edge (xpbd_query_grid.hip): 2 x the largest bounding radius of the shapes in use x (1 + 1e-6), the
    radius as xpbd_world_set_polytopes computes it."""
    rmax = 0.0
    for s in np.unique(sid):
        p = capi.scene_polytopes(kind)[int(s)]
        d = np.asarray(p["vertices"]) - np.asarray(p["centroid"])
        for v in d:
            rmax = max(rmax, float(np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])))
    return 2.0 * rmax * (1.0 + 1e-6)


def ray_families(rng, state, edge, n):
    """n rays, seven families of equal share, around the bodies of `state` (n x 38)."""
    centre = state[:, 31:34] + state[:, 28:31]
    lo, hi = centre.min(axis=0) - 2.0, centre.max(axis=0) + 2.0
    k = n // 7
    unit = lambda m: (lambda v: v / np.linalg.norm(v, axis=1, keepdims=True))(rng.normal(size=(m, 3)))
    parts = []
    # random rays inside the box, half of them with a finite reach
    o = rng.uniform(lo, hi, size=(k, 3))
    parts.append(capi.rays(o, unit(k), max_distance=np.where(rng.random(k) < 0.5, np.inf, rng.uniform(0.0, 20.0, k))))
    # infinite rays from outside the box, aimed at points inside it
    mid, radius = 0.5 * (lo + hi), 0.6 * np.linalg.norm(hi - lo)
    o = mid + radius * unit(k)
    parts.append(capi.rays(o, rng.uniform(lo, hi, size=(k, 3)) - o))
    # a camera fan from above
    side = int(np.sqrt(k))
    u, v = np.meshgrid(np.linspace(-0.5, 0.5, side), np.linspace(-0.5, 0.5, side))
    eye = np.array([mid[0], mid[1], hi[2] + 30.0])
    d = np.stack([u.ravel() * (hi[0] - lo[0]) / 30.0, v.ravel() * (hi[1] - lo[1]) / 30.0, -np.ones(side * side)], axis=1)
    parts.append(capi.rays(np.broadcast_to(eye, d.shape), d))
    # rays starting inside bodies
    pick = rng.integers(0, len(state), k)
    parts.append(capi.rays(centre[pick] + rng.uniform(-0.05, 0.05, (k, 3)), unit(k)))
    # axis-aligned rays
    axes = np.eye(3)[rng.integers(0, 3, k)] * rng.choice([-1.0, 1.0], (k, 1))
    parts.append(capi.rays(rng.uniform(lo, hi, size=(k, 3)), axes))
    # rays lying in cell faces: two coordinates on multiples of the cell edge, moving along the third axis
    o = rng.uniform(lo, hi, size=(k, 3))
    axis = rng.integers(0, 3, k)
    for a in range(3):
        on = axis != a
        o[on, a] = np.floor(o[on, a] / edge) * edge
    parts.append(capi.rays(o, np.eye(3)[axis] * rng.choice([-1.0, 1.0], (k, 1))))
    # rays from a body's centre outwards that ignore that body
    rest = n - sum(len(p) for p in parts)
    pick = rng.integers(0, len(state), rest)
    parts.append(capi.rays(centre[pick], unit(rest), ignore=pick))
    return np.concatenate(parts)


def check_grid_equals_brute(w, state, kind, sid, seed, n_rays=65536, fan=512, dense=True):
    rng = np.random.default_rng(seed)
    r = ray_families(rng, state, cell_edge(kind, sid), n_rays)
    grid, brute = w.raycast(r), w.raycast(r, BRUTE)
    assert same_bits(grid, brute)
    assert 0.1 < np.mean(grid["body"] != capi.NO_HIT) < 1.0
    assert np.any(grid["face"] == capi.RAY_INSIDE)
    assert np.any((grid["face"] != capi.RAY_INSIDE) & (grid["body"] != capi.NO_HIT)) or not dense
    # the ignore_body family never names the body it ignores
    tail = r["ignore_body"] != capi.NO_HIT
    assert not np.any(grid["body"][tail] == r["ignore_body"][tail])
    # a 512 x 512 camera fan from above
    centre = state[:, 31:34] + state[:, 28:31]
    lo, hi = centre.min(axis=0), centre.max(axis=0)
    u, v = np.meshgrid(np.linspace(lo[0], hi[0], fan), np.linspace(lo[1], hi[1], fan))
    eye = np.array([0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), hi[2] + 50.0])
    targets = np.stack([u.ravel(), v.ravel(), np.full(fan * fan, lo[2])], axis=1)
    r = capi.rays(np.broadcast_to(eye, targets.shape), targets - eye)
    grid, brute = w.raycast(r), w.raycast(r, BRUTE)
    assert same_bits(grid, brute)
    assert np.mean(grid["body"] != capi.NO_HIT) > 0.05 or not dense


def test_grid_equals_brute_force_on_the_settled_box_pile():
    n = 262144
    bodies, sid = capi.scene_pile(capi.SCENE_BOXES_DROP, 1, n, 2.0, 4)
    w = stepped(bodies, sid, capi.SCENE_BOXES_DROP, 90)
    try:
        state = w.download()
        assert not np.isnan(state).any()
        check_grid_equals_brute(w, state, capi.SCENE_BOXES_DROP, sid, 1)
    finally:
        w.close()


def test_grid_equals_brute_force_on_the_mixed_pile():
    n = 65536
    bodies, sid = capi.scene_pile(capi.SCENE_MIXED_DROP, 1, n, 1.4, 4)
    w = stepped(bodies, sid, capi.SCENE_MIXED_DROP, 45)
    try:
        state = w.download()
        check_grid_equals_brute(w, state, capi.SCENE_MIXED_DROP, sid, 2)
    finally:
        w.close()


def test_grid_equals_brute_force_on_a_sparse_hashed_world():
    """4 096 bodies spread over a 4 km cube: far more cells than the table has buckets, so the grid is hashed."""
    rng = np.random.default_rng(3)
    n = 4096
    bodies, sid = capi.scene_generate(capi.SCENE_MIXED_DROP, 3, n)
    bodies[:, 31:34] = rng.uniform(-2000.0, 2000.0, (n, 3))
    with capi.World(mode=capi.MODE_FUSED) as w:
        w.set_polytopes(capi.scene_polytopes(capi.SCENE_MIXED_DROP))
        w.upload(bodies, sid)
        check_grid_equals_brute(w, bodies, capi.SCENE_MIXED_DROP, sid, 3, n_rays=16384, fan=128, dense=False)
        # rays aimed at bodies, so that this world is not mostly misses
        centre = bodies[:, 31:34] + bodies[:, 28:31]
        o = centre + rng.normal(size=(n, 3)) * 50.0
        r = capi.rays(o, centre - o)
        grid, brute = w.raycast(r), w.raycast(r, BRUTE)
        assert same_bits(grid, brute) and np.mean(grid["body"] != capi.NO_HIT) > 0.9


def small_pile(n=2048):
    bodies, sid = capi.scene_pile(capi.SCENE_MIXED_DROP, 7, n, 1.4, 2)
    return bodies, sid


@pytest.mark.parametrize("mode", [capi.MODE_FUSED, capi.MODE_PER_SUBSTEP, capi.MODE_CONTACTS])
def test_device_equals_the_model_after_stepping(mode):
    bodies, sid = small_pile()
    polys = capi.scene_polytopes(capi.SCENE_MIXED_DROP)
    w = stepped(bodies, sid, capi.SCENE_MIXED_DROP, 25, substeps=10, mode=mode)
    try:
        state = w.download()
        rng = np.random.default_rng(10 + mode)
        r = ray_families(rng, state, cell_edge(capi.SCENE_MIXED_DROP, sid), 2048)
        got = w.raycast(r)
    finally:
        w.close()
    want, second = rm.raycast(state, sid, polys, r)
    assert np.mean(want["body"] != rm.NO_HIT) > 0.2
    best = want["distance"]
    with np.errstate(invalid="ignore"):                             # (inf - inf: no second candidate)
        clear = ~(np.abs(second - best) <= 1e-9 * np.maximum(np.abs(best), 1.0))
    np.testing.assert_array_equal(got["body"][clear], want["body"][clear])
    np.testing.assert_array_equal(got["face"][clear], want["face"][clear])
    hit = clear & (want["body"] != rm.NO_HIT)
    for key, width in (("distance", None), ("point", 3), ("normal", 3)):
        g, m = got[key][hit], want[key][hit]
        np.testing.assert_allclose(g, m, rtol=1e-12, atol=1e-12)
    # the model keeps the kernel's operation order: the same bits
    assert same_bits(got["distance"][hit], want["distance"][hit])
    assert same_bits(got["point"][hit], want["point"][hit]) and same_bits(got["normal"][hit], want["normal"][hit])


def test_a_ray_cast_has_no_side_effects():
    bodies, sid = small_pile(4096)
    rng = np.random.default_rng(5)
    worlds = []
    for cast in (False, True):
        w = capi.World(mode=capi.MODE_CONTACTS, trace_contacts=True)
        w.set_polytopes(capi.scene_polytopes(capi.SCENE_MIXED_DROP))
        w.upload(bodies, sid)
        for f in range(30):
            w.step(DT, 10)
            if cast:
                w.raycast(ray_families(rng, bodies, 1.0, 4096))
                w.raycast(capi.rays([[0.0, 0.0, 50.0]], [[0.0, 0.0, -1.0]]))     # the brute-force path of a handful of rays
        worlds.append((w.download(), w.contacts(), w.contact_masks(10)))
        w.close()
    for a, b in zip(*worlds):
        assert same_bits(a, b)


def test_device_variant_on_a_caller_stream_equals_the_host_variant(tmp_path):
    """torch tensors on a torch stream handed to the world with set_stream.  In a child process that imports torch first: the
    library then binds to the HIP runtime torch carries, as in bench.py (in this process it already has its own)."""
    import json
    import os
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    code = r'''
import sys, json
sys.path[:0] = [%r, %r]
import numpy as np, torch
torch.cuda.set_device(0)
from constraint_solver_amd import capi
import test_gpu_raycast as t
bodies, sid = t.small_pile(4096)
w = t.stepped(bodies, sid, capi.SCENE_MIXED_DROP, 10, substeps=10)
r = t.ray_families(np.random.default_rng(6), w.download(), 1.0, 8192)
stream = torch.cuda.Stream()
w.set_stream(stream.cuda_stream)
res = {}
with torch.cuda.stream(stream):
    dev_rays = torch.from_numpy(r.view(np.uint8).copy()).to("cuda")
    for flags in (0, t.BRUTE):
        dev_hits = torch.zeros(len(r) * 64, dtype=torch.uint8, device="cuda")
        w.raycast_device(dev_rays.data_ptr(), len(r), dev_hits.data_ptr(), flags)
        got = dev_hits.cpu().numpy().view(capi.RAY_HIT_DTYPE)          # (ordered after the cast on the same stream)
        res[str(flags)] = t.same_bits(got, w.raycast(r)) and bool(np.any(got["body"] != capi.NO_HIT))
w.set_stream(0)
w.close()
print(json.dumps(res))
''' % (os.path.dirname(here), here)
    script = tmp_path / "child.py"
    script.write_text(code)
    out = subprocess.run([sys.executable, str(script)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res == {"0": True, "1": True}


@pytest.mark.parametrize("n_ranks", [2, 4])
def test_sharded_world_equals_the_single_world(n_ranks):
    n, frames, substeps = 65536, 30, 10
    kind = capi.SCENE_MIXED_DROP
    bodies, sid = capi.scene_pile(kind, 1, n, 1.4, 4)
    single = stepped(bodies, sid, kind, frames, substeps)
    with capi.MultiWorld(n_ranks, devices=[0] * n_ranks, transport=capi.TRANSPORT_LOCAL, halo_margin=0.75, auto_replan=True) as mw:
        mw.set_polytopes(capi.scene_polytopes(kind))
        mw.upload(bodies, sid, 0, n)
        for _ in range(frames):
            mw.step(DT, substeps)
        state = single.download()
        r = ray_families(np.random.default_rng(20 + n_ranks), state, cell_edge(kind, sid), 16384)
        want = single.raycast(r)
        assert same_bits(mw.raycast(r[:256]), want[:256])   # under the plans the steps made; then under one more
        mw.replan()
        assert mw.plan_stats()["plans"] >= 2
        assert same_bits(mw.download(), state)
        assert same_bits(mw.raycast(r), want)
        assert same_bits(mw.raycast(r, BRUTE), want)
        assert same_bits(mw.raycast(r[:3]), want[:3])
    single.close()


def test_argument_errors():
    r = capi.rays([[0.0, 0.0, 5.0]], [[0.0, 0.0, -1.0]])
    with capi.World(mode=capi.MODE_FUSED) as w:
        verts, off = capi.scene_shapes(capi.SCENE_BOXES)
        w.set_shapes(verts, off)
        w.upload(*capi.scene_generate(capi.SCENE_BOXES, 1, 4))
        with pytest.raises(capi.XpbdError, match="set_polytopes") as e:
            w.raycast(r)                                             # vertices only
        assert e.value.code == capi.E_INVALID
    bodies, sid = small_pile(64)
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(capi.SCENE_MIXED_DROP))
        w.upload(bodies, sid)
        assert w.raycast(r[:0]).size == 0                           # n_rays = 0 is OK
        bad = r.copy()
        bad["reserved"] = 1
        with pytest.raises(capi.XpbdError, match="reserved"):
            w.raycast(bad)
        with pytest.raises(capi.XpbdError, match="unknown flags"):
            w.raycast(r, 2)
        L = capi.hip_lib()
        assert L.xpbd_world_raycast(w._h, None, 1, 0, None) == capi.E_INVALID
        assert L.xpbd_world_raycast_device(w._h, None, 1, 0, None) == capi.E_INVALID
    with capi.MultiWorld(2, devices=[0, 0], transport=capi.TRANSPORT_LOCAL) as mw:
        with pytest.raises(capi.XpbdError, match="set_polytopes"):
            mw.raycast(r)
        mw.set_polytopes(capi.scene_polytopes(capi.SCENE_MIXED_DROP))
        with pytest.raises(capi.XpbdError, match="no bodies"):
            mw.raycast(r)
        mw.upload(bodies, sid, 0, len(bodies))
        with pytest.raises(capi.XpbdError, match="unknown flags"):
            mw.raycast(r, 4)
        with pytest.raises(capi.XpbdError, match="reserved"):
            mw.raycast(bad)
        assert mw.raycast(r[:0]).size == 0


def test_worlds_and_shards_without_bodies():
    """A world without bodies and a sharded world with empty shards: every ray that finds nothing misses (grid-sized batches)."""
    rng = np.random.default_rng(8)
    kind = capi.SCENE_MIXED_DROP
    bodies, sid = small_pile(3)
    r = ray_families(rng, bodies, 1.0, 4096)
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(kind))
        w.upload(bodies[:0], sid[:0])
        for flags in (0, BRUTE):
            got = w.raycast(r, flags)
            assert (got["body"] == capi.NO_HIT).all() and (got["distance"] == np.inf).all()
        w.upload(bodies, sid)
        want = w.raycast(r)
    assert np.any(want["body"] != capi.NO_HIT)
    with capi.MultiWorld(4, devices=[0] * 4, transport=capi.TRANSPORT_LOCAL) as mw:   # three bodies, four shards
        mw.set_polytopes(capi.scene_polytopes(kind))
        mw.upload(bodies, sid, 0, len(bodies))
        assert same_bits(mw.raycast(r), want)
