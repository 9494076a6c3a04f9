"""k_step's grid path against the CPU oracle, bit for bit.

A uniform wave of an 8-vertex shape whose table is a *bounded grid table* -- vertex v = (X[v & 1], Y[(v >> 1) & 1],
Z[(v >> 2) & 1]) as 64-bit patterns, the six values below 2^970 in magnitude -- runs pass 1 from the six values and takes
`frame * vertex` with one fma for the closing `c * 2 + v` (DESIGN sections 2 and 4).  Every other 8-vertex table keeps the
general copy of the loop.  Here: tables on both sides of every clause of that test (unit cube, a cuboid of six different
coordinates, +0.0 against -0.0, two vertices swapped, one coordinate off by an ulp, a frustum, a coordinate of 2^969 and
one of 2^971), grid and non-grid shapes in neighbouring waves, a mixed wave, a one-lane tail wave and a NaN height; bodies
in, above and rocking on the ground; 1, 3 and 20 substeps; contact trace on and off (both instantiations of the kernel).
All 13 dynamic doubles of every body (and the 25 static ones) and every substep's contact mask are compared."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
from constraint_solver_amd import capi
from golden_util import bits_equal

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
FRAMES = 2
POS_Z = 33
ULP1 = np.nextafter(1.0, 2.0)


def grid(xs, ys, zs):
    """The box (xs) x (ys) x (zs) in binary vertex order, v = x + 2 y + 4 z."""
    return np.array([[xs[v & 1], ys[(v >> 1) & 1], zs[(v >> 2) & 1]] for v in range(8)], dtype=np.float64)


def is_bounded_grid_table(t):
    """The kernel's test, restated: 64-bit patterns against the table rebuilt from its six values, and the 2^970 bound."""
    t = np.ascontiguousarray(t, dtype=np.float64).reshape(8, 3)
    six = (t[[0, 1], 0], t[[0, 2], 1], t[[0, 4], 2])
    same = np.array_equal(grid(*six).view(np.uint64), t.view(np.uint64))
    return bool(same and all((np.abs(s) < 2.0 ** 970).all() for s in six))      # a NaN fails `<`


def _swapped(t, a, b):
    t = t.copy()
    t[[a, b]] = t[[b, a]]
    return t


def _moved(t, v, axis, value):
    t = t.copy()
    t[v, axis] = value
    return t


CUBE = capi.scene_shapes(capi.SCENE_BOXES)[0]
CUBOID = grid((-0.75, 0.5), (-0.25, 1.5), (-0.125, 0.875))
# (shape table, takes the grid path)
SHAPES = {
    "cube": (CUBE, True),
    "cuboid": (CUBOID, True),
    "signed_zeros": (_moved(grid((0.0, 1.0), (0.0, 1.0), (0.0, 1.0)), 2, 0, -0.0), False),   # +0.0 in vertex 0, -0.0 in vertex 2
    "swapped": (_swapped(CUBE, 1, 2), False),
    "ulp": (_moved(grid((0.0, 1.0), (0.0, 1.0), (0.0, 1.0)), 7, 2, ULP1), False),
    "sheared": (grid((0.0, 1.0), (0.0, 1.0), (0.0, 1.0)) + np.outer(grid((0, 0), (0, 0), (0.0, 0.5))[:, 2], [1.0, 0.0, 0.0]), False),
    "frustum": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0], [0.25, 0.25, 1], [0.75, 0.25, 1], [0.25, 0.75, 1],
                          [0.75, 0.75, 1]], dtype=np.float64), False),
    "huge_2p969": (grid((-0.5, 2.0 ** 969), (-0.25, 1.5), (-0.125, 0.875)), True),
    "huge_2p971": (grid((-0.5, 2.0 ** 971), (-0.25, 1.5), (-0.125, 0.875)), False),
}
NAMES = sorted(SHAPES)
VERTS = np.concatenate([SHAPES[k][0] for k in NAMES])
OFFSETS = (8 * np.arange(len(NAMES) + 1)).astype(np.uint32)
ID = {k: i for i, k in enumerate(NAMES)}


def _bodies(n, seed):
    """SCENE_BOXES bodies (random rotations, heights around the ground): every fifth lifted clear, every fifth pushed in."""
    bodies, _ = capi.scene_generate(capi.SCENE_BOXES, seed, n)
    bodies[:, POS_Z] *= 0.25                           # the generator's [-0.05, 0.55) closer to the ground: most corners touch at once
    bodies[1::5, POS_Z] += 10.0
    bodies[3::5, POS_Z] = -3.0
    return bodies


def _uniform(n, shape, seed):
    return _bodies(n, seed), np.full(n, ID[shape], dtype=np.uint32)


def _one_cube(seed):
    bodies, sid = _uniform(1, "cube", seed)
    bodies[0, POS_Z] = 0.0                             # rocking on the ground from the first substep
    return bodies, sid


def _neighbours(seed):
    bodies, sid = _uniform(130, "cube", seed)          # wave 0 grid, wave 1 general, a two-lane tail wave of another grid shape
    sid[64:128] = ID["swapped"]
    sid[128:] = ID["cuboid"]
    return bodies, sid


def _odd_lane(seed):
    bodies, sid = _uniform(64, "cube", seed)           # two grid shapes in one wave: mixed, the per-lane walk
    sid[17] = ID["cuboid"]
    return bodies, sid


def _nan_height(seed):
    bodies, sid = _uniform(64, "cube", seed)
    bodies[6, POS_Z] = np.nan
    return bodies, sid


SCENES = {
    "cube_1": lambda: _one_cube(21),
    "cube_65": lambda: _uniform(65, "cube", 22),                   # a full wave and a one-lane tail wave
    "cuboid_63": lambda: _uniform(63, "cuboid", 23),
    "signed_zeros_64": lambda: _uniform(64, "signed_zeros", 24),
    "swapped_64": lambda: _uniform(64, "swapped", 25),
    "ulp_65": lambda: _uniform(65, "ulp", 26),
    "sheared_63": lambda: _uniform(63, "sheared", 27),
    "frustum_64": lambda: _uniform(64, "frustum", 28),
    "neighbours_130": lambda: _neighbours(29),
    "odd_lane_64": lambda: _odd_lane(30),
    "nan_height_64": lambda: _nan_height(31),
    "huge_2p969_64": lambda: _uniform(64, "huge_2p969", 32),
    "huge_2p971_64": lambda: _uniform(64, "huge_2p971", 33),
}
# where NaN (or inf - inf) is expected: NaN-ness is compared, and bits wherever the value is no NaN
MAY_HOLD_NAN = {"nan_height_64", "huge_2p969_64", "huge_2p971_64"}


@functools.lru_cache(maxsize=None)
def scene_and_oracle(name, substeps):
    """(bodies, shape ids, oracle bodies per frame, oracle masks [FRAMES][substeps][n]); computed once, read-only."""
    bodies, sid = SCENES[name]()
    want, states, masks = bodies, [], []
    for _ in range(FRAMES):
        want, m = ob.step_bodies(want, sid, VERTS, OFFSETS, DT, substeps, want_masks=True, threads=4)
        states.append(want)
        masks.append(m)
    states, masks = np.array(states), np.array(masks)
    for a in (bodies, sid, states, masks):
        a.setflags(write=False)
    return bodies, sid, states, masks


def same_bits_or_both_nan(got, want):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and \
        np.array_equal(got.view(np.uint64)[~nan], want.view(np.uint64)[~nan])


def test_tables_fall_on_the_intended_side_of_the_grid_test():
    """No GPU arithmetic: the restated predicate on every table, and the library's cube is in binary vertex order."""
    for name, (table, want_grid) in SHAPES.items():
        assert table.shape == (8, 3)
        assert is_bounded_grid_table(table) == want_grid, name
    six = {CUBOID[0, 0], CUBOID[1, 0], CUBOID[0, 1], CUBOID[2, 1], CUBOID[0, 2], CUBOID[4, 2]}
    assert len(six) == 6 and min(six) < 0.0
    z = SHAPES["signed_zeros"][0]
    assert z[0, 0] == 0.0 == z[2, 0] and not np.signbit(z[0, 0]) and np.signbit(z[2, 0])
    assert SHAPES["ulp"][0][7, 2] == ULP1 and sorted(map(tuple, SHAPES["swapped"][0])) == sorted(map(tuple, CUBE))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_reaches_its_case(name):
    """What each scene is there for holds in the oracle's own masks."""
    bodies, sid, states, masks = scene_and_oracle(name, 3)
    count = np.array([bin(m).count("1") for m in masks[0, 0]])
    n = len(sid)
    assert (count > 0).any()                                           # pass 2 runs in the first substep
    if n >= 63:
        assert (count == 0).any() and (count == 8).any() and len(set(count)) >= 4   # above, in, and rocking on the ground
    if name == "neighbours_130":
        assert [len(set(sid[a:b])) for a, b in ((0, 64), (64, 128), (128, 130))] == [1, 1, 1] and len(set(sid)) == 3
    if name == "odd_lane_64":
        assert list(np.flatnonzero(sid != ID["cube"])) == [17]
    if name == "nan_height_64":
        assert (masks[:, :, 6] == 0xFF).all() and np.isnan(states[-1][6, POS_Z])    # every vertex a contact, as in the reference
    if name not in MAY_HOLD_NAN:
        assert not np.isnan(states).any()


@pytest.mark.parametrize("trace", [True, False])
@pytest.mark.parametrize("substeps", [1, 3, 20])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_grid_table_path_vs_oracle(name, substeps, trace):
    bodies, sid, states, masks = scene_and_oracle(name, substeps)
    same = same_bits_or_both_nan if name in MAY_HOLD_NAN else bits_equal
    with capi.World(mode=capi.MODE_FUSED, trace_contacts=trace) as w:
        w.set_shapes(VERTS, OFFSETS)
        w.upload(bodies, sid)
        for f in range(FRAMES):
            w.step(DT, substeps)
            if trace:
                assert np.array_equal(w.contact_masks(substeps), masks[f]), "contact masks differ in frame %d" % f
            assert same(w.download(), states[f]), "bodies differ in frame %d" % f
        contacts = w.contacts()
    assert np.array_equal(contacts, ob.masks_to_contacts(masks[-1][-1]))
