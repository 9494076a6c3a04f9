"""Island sleeping on the schedules and kernel forms the plain scenes of test_gpu_sleeping.py never reach: the per-substep
schedule of a world with restitution (the velocity pass runs over everybody and the sleepers are put back) or with a terrain,
the neighbour kernels' forms that test collision filters and the inert table together, and the contact trace.  Each scene is
held to the same three checks: the library's state equals the model's after every frame, a sleeper is bit-frozen and no report
pair has two inert ends, and a twin that never sleeps is the same bits until the first island sleeps (and, for a body far from
every sleeper, for as long as it stays awake)."""
import numpy as np
import pytest

import islands_model as im
import sleep_common as sc
from constraint_solver_amd import capi

pytestmark = pytest.mark.gpu


def dropper_world(sleeping, setup):
    w, joints = sc.stack_world(True, sc.CFG if sleeping else None)
    setup(w)
    return w, joints


def bouncy(w):
    # every contact that closes faster than 1 m/s bounces: the dropped box and the falling one do, the stack's jitter does not
    w.set_restitution(np.full(w.n, 0.4), ground_restitution=0.4, bounce_threshold=1.0)


def flat_terrain(w):
    # z = 0 as a heightfield under the whole scene (x -10..56, y -10..11)
    w.set_terrain(np.zeros((4, 12)), origin=(-10.0, -10.0), cell=(6.0, 7.0))


@pytest.mark.parametrize("name,setup,frames", [("restitution", bouncy, 450), ("terrain", flat_terrain, 200),
                                               ("restitution on a terrain", lambda w: (bouncy(w), flat_terrain(w)), 200)])
def test_the_per_substep_schedule_with_sleepers(name, setup, frames):
    run, twin = sc.run_with_twin(lambda on: dropper_world(on, setup), frames)
    slept_at = next(k + 1 for k, f in enumerate(run) if f.asleep[0])
    woken_at = next((k + 1 for k, f in enumerate(run) if k + 1 > slept_at and not f.asleep[0]), None)
    frozen = sc.assert_frozen(run)
    compared = sc.assert_twin(run, twin, (sc.FALLING,))
    print("%s: stack asleep in frame %d, woken in frame %s, %d frozen (body, frame), %d twin rows, asleep at the end %s"
          % (name, slept_at, woken_at, frozen, compared, run[-1].sleep_counts[:2]))
    assert 30 <= slept_at <= 60 and woken_at is not None     # the dropped box lands on the sleeping stack
    assert run[woken_at - 1].sleep_counts[2] == 3            # and wakes all of it in one pass
    assert frozen > 100 and compared >= 120
    if "restitution" in name:                                # the scene does bounce: the twin differs from a world without restitution
        plain, _ = sc.stack_world(True, None)
        with plain:
            for _ in range(75):
                plain.step(sc.DT, sc.SUBSTEPS)
            assert not im.same_bytes(plain.download()[sc.DROPPER], twin[74].bodies[sc.DROPPER])


def filtered_drop_world(sleeping, filters, flags):
    w, joints = sc.drop_world(sleeping=sc.LOOSE if sleeping else None)
    w.set_collision_filters(filters(w.n) if filters else None, flags)
    return w, joints


def some_filters(n):
    """Three groups; every fifth body ignores the next group: some neighbouring boxes pass through each other."""
    i = np.arange(n)
    f = np.zeros(n, dtype=capi.COLLISION_FILTER_DTYPE)
    f["group"] = np.uint32(1) << (i % 3).astype(np.uint32)
    f["mask"] = np.where(i % 5 == 0, np.uint32(0xFFFFFFFF) ^ (np.uint32(1) << ((i + 1) % 3).astype(np.uint32)), np.uint32(0xFFFFFFFF))
    return f


@pytest.mark.parametrize("name,filters,flags", [("group and mask", some_filters, 0), ("jointed pairs", None, capi.FILTER_JOINTED),
                                                ("group, mask and jointed pairs", some_filters, capi.FILTER_JOINTED)])
def test_box_drop_with_collision_filters(name, filters, flags):
    """The neighbour kernels' forms that test the filters and the inert table together; the fixed bodies 5 and 200 are inert too."""
    run, twin = sc.run_with_twin(lambda on: filtered_drop_world(on, filters, flags), 120, cfg=sc.LOOSE, substeps=10)
    frozen = sc.assert_frozen(run)
    sc.assert_twin(run, twin)
    slept, woken = sum(f.sleep_counts[3] for f in run), sum(f.sleep_counts[2] for f in run)
    print("%s: put to sleep %d, woken %d, %d frozen (body, frame), pairs at the end %d (twin %d)"
          % (name, slept, woken, frozen, run[-1].counts[0], twin[-1].counts[0]))
    assert slept > 100 and woken > 0 and frozen > 100
    if filters:                                              # the group / mask filters are in force: the plain drop ends elsewhere
        plain, _ = sc.drop_world(sleeping=None)
        with plain:
            for _ in range(120):
                plain.step(sc.DT, 10)
            assert not im.same_bytes(plain.download(), twin[-1].bodies)


def test_trace_rows_of_a_sleeper_repeat_its_frozen_mask():
    w, joints = sc.stack_world(False, sc.CFG, trace=True)
    t, _ = sc.stack_world(False, None, trace=True)
    state = None
    rows_checked = 0
    with w, t:
        asleep = np.zeros(w.n, dtype=bool)
        for k in range(1, 71):
            before = im.masks_from_contacts(w.n, w.contacts()) if k > 1 else np.zeros(w.n, dtype=np.uint32)
            frames, state = sc.run_against_model(w, joints, sc.CFG, 1, state=state, first_frame=k)
            t.step(sc.DT, sc.SUBSTEPS)
            trace, twin_trace = w.contact_masks(sc.SUBSTEPS), t.contact_masks(sc.SUBSTEPS)
            after = im.masks_from_contacts(w.n, frames[0].contacts)
            assert trace.shape == (sc.SUBSTEPS, w.n) and np.array_equal(trace[-1], after), k     # the last row is the mask the download shows
            for i in np.flatnonzero(asleep):                 # asleep during this frame: every row is the mask it fell asleep with
                assert np.all(trace[:, i] == before[i]) and after[i] == before[i], (k, i)
                rows_checked += sc.SUBSTEPS
            awake = ~asleep
            if not asleep.any():
                assert np.array_equal(trace, twin_trace), k  # nobody asleep yet: the twin's trace
            else:
                assert np.array_equal(trace[:, sc.FALLING], twin_trace[:, sc.FALLING]), k
            assert awake[sc.FALLING]
            asleep = frames[0].asleep.astype(bool)
    assert asleep[list(sc.STACK)].all() and asleep[sc.SINGLE] and rows_checked > 20 * sc.SUBSTEPS
    assert before[0] != 0 and before[sc.SINGLE] != 0        # the bottom box and the single box rest on the ground: a mask worth repeating
