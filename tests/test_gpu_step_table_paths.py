"""The three ways k_step reads the shape vertex table, each against the CPU oracle bit for bit.

A wave whose live lanes share one shape takes a uniform path: 4 or 8 vertices are held in scalar registers, any other
count stays in LDS and is walked by a scalar-counted loop.  A wave of several shapes keeps the per-lane walk.  Pass 2
is the same on all of them: each lane reads its own penetrating vertices from LDS.  The scenes are the smallest that
reach each path and its edges:
a one-lane tail wave, a partial workgroup (dead lanes must not vote), one odd lane in an otherwise uniform wave, and
trip counts from 0 to 8 in one wave.  Every scene starts in or next to ground contact, so pass 2 runs from the first
substep; 3 frames x 20 substeps, both kernel instantiations (contact trace on / off), fused and per-substep launches,
workgroups of 64 and 256."""
import functools

import numpy as np
import pytest

import oracle_binding as ob
from constraint_solver_amd import capi
from golden_util import bits_equal

pytestmark = pytest.mark.gpu

DT = 1.0 / 60.0
SUBSTEPS, FRAMES = 20, 3
CUBE, TETRAHEDRON, ICOSAHEDRON = capi.SHAPE_CUBE, capi.SHAPE_TETRAHEDRON, capi.SHAPE_ICOSAHEDRON
POS_Z = 33


def _boxes(n, seed):
    bodies, _ = capi.scene_generate(capi.SCENE_BOXES, seed, n)
    return bodies, np.full(n, CUBE, dtype=np.uint32)


def _one_shape(n, shape, seed):
    bodies, _ = capi.scene_generate(capi.SCENE_MIXED, seed, n)
    return bodies, np.full(n, shape, dtype=np.uint32)


def _interleaved(n, seed):
    bodies, _ = capi.scene_generate(capi.SCENE_MIXED, seed, n)
    return bodies, (np.arange(n) % 3).astype(np.uint32)


def _boxes_last_lane_tetrahedron(seed):
    bodies, sid = _boxes(64, seed)
    sid[63] = TETRAHEDRON
    return bodies, sid


def _boxes_trips_0_to_8(seed):
    bodies, sid = _boxes(64, seed)
    bodies[5, POS_Z] += 10.0          # airborne: no trip
    bodies[40, POS_Z] = -3.0          # the whole box below the plane: 8 trips
    return bodies, sid


SCENES = {
    "boxes_65": lambda: _boxes(65, 11),                                   # a full scalar-table wave + a one-lane wave
    "tetrahedra_64": lambda: _one_shape(64, TETRAHEDRON, 12),             # scalar table, 4 vertices
    "icosahedra_64": lambda: _one_shape(64, ICOSAHEDRON, 13),             # 12 vertices: uniform loop over LDS
    "interleaved_128": lambda: _interleaved(128, 14),                     # every wave mixed: the per-lane walk
    "boxes_64_last_lane_tetrahedron": lambda: _boxes_last_lane_tetrahedron(15),   # must be found mixed
    "boxes_127": lambda: _boxes(127, 16),                                 # partial workgroup at 256
    "boxes_64_trips_0_to_8": lambda: _boxes_trips_0_to_8(17),
}


@functools.lru_cache(maxsize=None)
def scene_and_oracle(name):
    """(bodies, shape ids, verts, offsets, oracle poses after FRAMES, oracle masks [FRAMES][SUBSTEPS][n]); computed once."""
    verts, off = capi.scene_shapes(capi.SCENE_MIXED)      # cube, tetrahedron, icosahedron
    assert list(np.diff(off)) == [8, 4, 12]
    bodies, sid = SCENES[name]()
    want, want_masks = bodies, []
    for _ in range(FRAMES):
        want, m = ob.step_bodies(want, sid, verts, off, DT, SUBSTEPS, want_masks=True, threads=4)
        want_masks.append(m)
    want_masks = np.array(want_masks)
    for a in (bodies, sid, want, want_masks):
        a.setflags(write=False)
    return bodies, sid, verts, off, want, want_masks


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scene_reaches_its_case(name):
    """What each scene is there for holds in the oracle's own masks (no GPU arithmetic involved)."""
    _, sid, _, _, _, masks = scene_and_oracle(name)
    count = np.array([bin(m).count("1") for m in masks[0, 0]])
    assert (count > 0).any()                                       # pass 2 runs in the first substep
    if name == "boxes_64_trips_0_to_8":
        assert count[5] == 0 and count[40] == 8 and len(set(sid)) == 1
    if name == "boxes_64_last_lane_tetrahedron":
        assert list(np.flatnonzero(sid != CUBE)) == [63]
    if name == "interleaved_128":
        assert all(len(set(sid[w:w + 64])) == 3 for w in (0, 64))


@pytest.mark.parametrize("block_size", [64, 256])
@pytest.mark.parametrize("mode", [capi.MODE_FUSED, capi.MODE_PER_SUBSTEP])
@pytest.mark.parametrize("trace", [True, False])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_table_path_vs_oracle(name, trace, mode, block_size):
    bodies, sid, verts, off, want, want_masks = scene_and_oracle(name)
    with capi.World(mode=mode, trace_contacts=trace, block_size=block_size) as w:
        w.set_shapes(verts, off)
        w.upload(bodies, sid)
        for f in range(FRAMES):
            w.step(DT, SUBSTEPS)
            if trace:
                assert np.array_equal(w.contact_masks(SUBSTEPS), want_masks[f]), "contact masks differ in frame %d" % f
        got, contacts = w.download(), w.contacts()
    assert bits_equal(got, want)
    assert np.array_equal(contacts, ob.masks_to_contacts(want_masks[-1][-1]))
