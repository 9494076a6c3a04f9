"""The native halo planner (csrc/xpbd_plan.cpp, the host-only unit behind xpbd_halo_plan) against the Python planner of
constraint_solver_amd/distributed.py, which the gloo tests pin to "sharded == single device": same ghosts, same boundary
bodies, for random clouds, piles, and joints that cross shard boundaries.  No GPU needed."""
import numpy as np
import pytest

from constraint_solver_amd import capi
from constraint_solver_amd.distributed import HaloPlan, bounding_spheres


def keys_of(centre, radius, pad, margin):
    edge = 2.0 * (float(radius.max()) + pad + margin)
    return np.array([capi.halo_cell_key(c, edge) for c in centre], dtype=np.int64)


@pytest.mark.parametrize("world_size", [2, 3, 5])
@pytest.mark.parametrize("case", ["line", "cloud", "pile", "joints"])
def test_native_plan_equals_python_plan(case, world_size):
    rng = np.random.default_rng(7)
    n = 997
    polys = capi.scene_polytopes(capi.SCENE_MIXED_DROP)
    radius = np.array([np.linalg.norm(p["vertices"] - p["centroid"], axis=1).max() for p in polys])
    centroid = np.array([p["centroid"] for p in polys])
    if case == "pile":
        bodies, sid = capi.scene_pile(capi.SCENE_MIXED_DROP, 3, n, 1.4, 3)
    else:
        bodies, sid = capi.scene_generate(capi.SCENE_MIXED_DROP, 3, n)
        if case == "cloud":
            bodies[:, 31:34] = rng.uniform(-6, 6, (n, 3))
    joints = None
    if case == "joints":
        a = rng.choice(n - 200, 40, replace=False)
        joints = np.zeros(40, dtype=capi.JOINT_DTYPE)
        joints["body_a"], joints["body_b"] = a, a + rng.integers(1, 200, 40)      # many cross shard boundaries, far apart
    centre, rad = bounding_spheres(bodies, sid, radius, centroid)
    pad, margin = 0.02, 0.75
    pairs = None if joints is None else np.stack([joints["body_a"], joints["body_b"]], axis=1).astype(np.int64)
    plan = HaloPlan(centre, rad, world_size, margin, pad, joint_pairs=pairs)
    keys = keys_of(centre, rad, pad, margin)
    total_ghosts = 0
    for rank in range(world_size):
        ghosts, boundary = capi.halo_plan(keys, world_size, rank, joints)
        assert np.array_equal(ghosts, np.sort(plan.ghosts[rank]))
        assert np.array_equal(boundary, plan.boundary[rank])
        total_ghosts += len(ghosts)
    assert total_ghosts > 0


def test_far_and_nan_centres_are_clamped_not_dropped():
    centre = np.array([[0.0, 0.0, 0.0], [1e30, 0.0, 0.0], [np.nan, 1.0, 1.0], [-1e30, -1e30, 5.0], [0.5, 0.5, 0.5]])
    keys = np.array([capi.halo_cell_key(c, 2.0) for c in centre], dtype=np.int64)
    assert keys[0] == keys[4] and len(set(keys.tolist())) == 4
    ghosts, boundary = capi.halo_plan(keys, 2, 0)                   # rank 0 owns bodies 0..2, rank 1 bodies 3, 4
    assert ghosts.tolist() == [4] and boundary.tolist() == [0]      # body 4 shares body 0's cell; the far ones reach nobody


def test_native_plan_is_conservative_and_symmetric():
    """Whatever the layout: (1) every remote body whose bounding sphere comes within 2 * (pad + margin) of an owned body's
    sphere is among the rank's ghosts -- nothing that could touch an owned body before the next plan is missing; (2) a body
    is on its owner's boundary list iff some other rank mirrors it (the all-gather rows and the ghost lists agree)."""
    rng = np.random.default_rng(5)
    n, world_size, pad, margin = 600, 4, 0.02, 0.25
    centre = rng.uniform(0, 14, (n, 3))
    radius = rng.uniform(0.3, 0.9, n)
    edge = 2.0 * (float(radius.max()) + pad + margin)
    keys = np.array([capi.halo_cell_key(c, edge) for c in centre], dtype=np.int64)
    reach = radius[:, None] + radius[None, :] + 2 * (pad + margin)
    close = np.linalg.norm(centre[:, None, :] - centre[None, :, :], axis=2) < reach
    base, extra = divmod(n, world_size)
    mirrored = np.zeros(n, dtype=bool)
    boundaries = []
    for rank in range(world_size):
        first = rank * base + min(rank, extra)
        count = base + (1 if rank < extra else 0)
        ghosts, boundary = capi.halo_plan(keys, world_size, rank)
        assert np.all(np.diff(ghosts.astype(np.int64)) > 0) and np.all(np.diff(boundary.astype(np.int64)) > 0)
        assert not np.any((ghosts >= first) & (ghosts < first + count)) and np.all((boundary >= first) & (boundary < first + count))
        present = set(ghosts.tolist()) | set(range(first, first + count))
        for i in range(first, first + count):
            assert set(np.nonzero(close[i])[0].tolist()) <= present
        mirrored[ghosts] = True
        boundaries.append(boundary)
    assert np.array_equal(np.nonzero(mirrored)[0], np.sort(np.concatenate(boundaries)))


@pytest.mark.parametrize("layout", ["cloud", "slabs"])
def test_far_bodies_are_more_than_two_cells_from_every_foreign_body(layout):
    """The larger travel allowance (halo_margin + half a cell edge) is only safe for a body with NO foreign body within two
    cells at plan time: checked by brute force; in a slab layout most interior bodies do get it."""
    rng = np.random.default_rng(11)
    n, world_size, edge = 800, (2 if layout == "slabs" else 4), (0.8 if layout == "slabs" else 1.7)
    centre = rng.uniform(0, 16, (n, 3))
    if layout == "slabs":
        centre = centre[np.argsort(centre[:, 1])]                   # index ranges = slabs along y
    keys = np.array([capi.halo_cell_key(c, edge) for c in centre], dtype=np.int64)
    cell = np.floor(centre / edge).astype(np.int64)
    base, extra = divmod(n, world_size)
    n_far = 0
    for rank in range(world_size):
        first = rank * base + min(rank, extra)
        count = base + (1 if rank < extra else 0)
        far = capi.halo_plan_far(keys, world_size, rank)
        assert len(far) == count
        foreign = np.ones(n, dtype=bool)
        foreign[first:first + count] = False
        for k in np.nonzero(far)[0]:
            gap = np.abs(cell[foreign] - cell[first + k]).max(axis=1)
            assert gap.min() >= 3
        n_far += int(far.sum())
    if layout == "slabs":
        assert n_far > 0.3 * n


# ---- ownership is the library's: the x-major cell sequence cut into runs of near-equal body count ---------------------------
def _cloud_keys(rng, n, extent, edge):
    centre = rng.uniform(0, extent, (n, 3)) * np.array([1.0, 0.4, 0.1])
    return centre, np.array([capi.halo_cell_key(c, edge) for c in centre], dtype=np.int64)


@pytest.mark.parametrize("world_size", [2, 3, 4, 8])
@pytest.mark.parametrize("n,extent,edge", [(2000, 60.0, 2.8), (997, 12.0, 2.8), (64, 1.0, 2.8), (5, 30.0, 2.8)])
def test_native_partition_equals_python_partition_and_is_balanced(world_size, n, extent, edge):
    from constraint_solver_amd.distributed import cell_keys, partition_owner
    rng = np.random.default_rng(n + world_size)
    centre, keys = _cloud_keys(rng, n, extent, edge)
    assert np.array_equal(keys, cell_keys(centre, edge))
    owner = capi.halo_partition(keys, world_size)
    assert np.array_equal(owner, partition_owner(keys, world_size))
    # slabs across the longest axis (x here): in (key, index) order the owners never decrease
    order = np.lexsort((np.arange(n), keys))
    assert np.all(np.diff(owner[order].astype(np.int64)) >= 0)
    # ... and for the same cloud turned so that y is its longest axis the bodies get the same owners
    turned = np.array([capi.halo_cell_key(c[[1, 0, 2]], edge) for c in centre], dtype=np.int64)
    assert np.array_equal(capi.halo_partition(turned, world_size), owner)
    assert np.array_equal(partition_owner(turned, world_size), owner)
    # balance: every cut lies within a quarter of a share of its ideal position
    counts = np.bincount(owner, minlength=world_size)
    assert counts.sum() == n
    share = max(1, n // world_size)
    ideal = np.array([n // world_size + (1 if r < n % world_size else 0) for r in range(world_size)])
    assert np.all(np.abs(np.cumsum(counts) - np.cumsum(ideal)) <= share / 4 + 1)
    # a cell is split between two ranks only where keeping it whole would have cost more than that
    if extent >= 12.0 and n >= 900:
        split = sum(len(set(owner[keys == k].tolist())) > 1 for k in np.unique(keys))
        assert split <= world_size - 1


def test_partition_does_not_depend_on_the_callers_numbering_of_cells():
    """The same bodies numbered differently: every CELL ends up with the same owner (only a split cell's bodies may differ)."""
    rng = np.random.default_rng(3)
    n, world_size = 3000, 4
    _, keys = _cloud_keys(rng, n, 80.0, 2.8)
    perm = rng.permutation(n)
    a, b = capi.halo_partition(keys, world_size), capi.halo_partition(keys[perm], world_size)
    whole = [k for k in np.unique(keys) if len(set(a[keys == k].tolist())) == 1]
    assert len(whole) > 0.95 * len(np.unique(keys))
    for k in whole:
        assert set(b[keys[perm] == k].tolist()) == set(a[keys == k].tolist())


@pytest.mark.parametrize("world_size", [2, 4])
def test_native_plan_with_library_owners_equals_python_plan(world_size):
    rng = np.random.default_rng(17)
    n = 1200
    polys = capi.scene_polytopes(capi.SCENE_MIXED_DROP)
    radius = np.array([np.linalg.norm(p["vertices"] - p["centroid"], axis=1).max() for p in polys])
    centroid = np.array([p["centroid"] for p in polys])
    bodies, sid = capi.scene_pile(capi.SCENE_MIXED_DROP, 3, n, 1.4, 3)
    perm = rng.permutation(n)                                      # the caller's numbering has nothing to do with space
    bodies, sid = bodies[perm], sid[perm]
    a = rng.choice(n - 200, 40, replace=False)
    joints = np.zeros(40, dtype=capi.JOINT_DTYPE)
    joints["body_a"], joints["body_b"] = a, a + rng.integers(1, 200, 40)
    centre, rad = bounding_spheres(bodies, sid, radius, centroid)
    pad, margin = 0.02, 0.5
    pairs = np.stack([joints["body_a"], joints["body_b"]], axis=1).astype(np.int64)
    plan = HaloPlan(centre, rad, world_size, margin, pad, joint_pairs=pairs, owner="library")
    keys = keys_of(centre, rad, pad, margin)
    owner = capi.halo_partition(keys, world_size)
    assert np.array_equal(owner, plan._owner)
    ghosts_index_ranges = 0
    for rank in range(world_size):
        ghosts, boundary, far = capi.halo_plan_owned(keys, owner, world_size, rank, joints, with_far=True)
        assert np.array_equal(ghosts, np.sort(plan.ghosts[rank]))
        assert np.array_equal(boundary, plan.boundary[rank])
        assert len(far) == len(plan.own_ids[rank]) and not np.any(far[np.isin(plan.own_ids[rank], boundary)])
        ghosts_index_ranges += len(capi.halo_plan(keys, world_size, rank, joints)[0])
    total = sum(len(g) for g in plan.ghosts)
    assert 0 < total < 0.5 * ghosts_index_ranges                   # slabs of space, not index ranges of a shuffled scene


@pytest.mark.parametrize("world_size", [2, 3, 5, 8])
@pytest.mark.parametrize("layout", ["flat", "cloud", "few cells", "tall"])
@pytest.mark.parametrize("motion", [0.0, 0.3, 2.5, 12.0])
def test_light_plan_equals_the_full_planner_after_any_motion(world_size, layout, motion):
    """A LIGHT plan (the re-plans of xpbd_multi_world: the cuts of the last full plan kept, every body still held by its old
    owner, only the RIMS of the shards known to everybody -- bodies within two layers of a cut, bodies that change owner, ends
    of joints that leave their holder) must give every rank exactly the lists the full planner computes from the keys and
    owners of the whole world: what it owns, its ghosts, its boundary bodies, its far flags.  Random worlds (a flat grid
    world, a 3-D cloud, a world of a handful of cells where cuts split cells, a tall one), random joints between arbitrary
    bodies, and bodies that have moved since the cut by nothing, a fraction of a cell, a cell, or many cells (several cuts)."""
    rng = np.random.default_rng(1000 * world_size + int(motion * 10) + len(layout))
    n, edge = 1500, 2.8
    extent = {"flat": (120.0, 60.0, 2.0), "cloud": (40.0, 30.0, 20.0), "few cells": (5.0, 4.0, 3.0), "tall": (6.0, 5.0, 200.0)}[layout]
    before = rng.uniform(0.0, 1.0, (n, 3)) * np.array(extent)
    after = before + rng.normal(0.0, 1.0, (n, 3)) * motion * edge / 2.0
    if motion:
        after[: n // 10] = rng.uniform(0.0, 1.0, (n // 10, 3)) * np.array(extent)        # and a tenth of them anywhere at all
    k0 = np.array([capi.halo_cell_key(c, edge) for c in before], dtype=np.int64)
    k1 = np.array([capi.halo_cell_key(c, edge) for c in after], dtype=np.int64)
    joints = np.zeros(120, dtype=capi.JOINT_DTYPE)
    a = rng.choice(n, 120, replace=False)
    b = (a + rng.integers(1, n, 120)) % n
    joints["body_a"], joints["body_b"] = a, b
    moved = 0
    for rank in range(world_size):
        owner, own, ghosts, boundary, far = capi.halo_plan_light(k0, k1, world_size, rank, joints)
        if rank == 0:
            moved = int((owner != capi.halo_partition(k0, world_size)).sum())
        assert np.array_equal(own, np.nonzero(owner == rank)[0])
        want_ghosts, want_boundary, want_far = capi.halo_plan_owned(k1, owner, world_size, rank, joints, with_far=True)
        assert np.array_equal(ghosts, want_ghosts) and np.array_equal(boundary, want_boundary) and np.array_equal(far, want_far)
    assert moved > 0 or motion == 0.0 or layout == "few cells"
