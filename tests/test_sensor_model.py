"""The occupancy model of the sensor tests (tests/sensor_model.py) against its brute-force restatement on random pair sets, and on
the hand-made cases the GPU tests lean on.  No device."""
import numpy as np

import sensor_model as sm
from constraint_solver_amd import capi


def random_case(rng, n, density, share):
    keys = sorted({(min(a, b), max(a, b)) for a, b in rng.integers(0, n, (int(density * n), 2)) if a != b})
    a = np.array([k[0] for k in keys], dtype=np.uint32)
    b = np.array([k[1] for k in keys], dtype=np.uint32)
    return a, b, (rng.random(n) < share).astype(np.uint8)


def test_occupancy_equals_the_brute_force_restatement_on_random_pair_sets():
    rng = np.random.default_rng(8100)
    listed = 0
    for case in range(200):
        n = int(rng.integers(1, 40))
        a, b, flags = random_case(rng, n, rng.uniform(0.0, 3.0), rng.choice([0.0, 0.1, 0.5, 1.0]))
        sensors, offsets, hits = sm.occupancy(a, b, flags)
        assert sm.as_lists(sensors, offsets, hits) == sm.brute_force(a, b, flags), case
        assert offsets[0] == 0 and offsets[-1] == len(hits) and len(offsets) == len(sensors) + 1
        for k in range(len(sensors)):
            mine = hits[offsets[k]:offsets[k + 1]]
            assert np.all(np.diff(mine["body"].astype(np.int64)) > 0)
            for h in mine:
                assert {int(a[h["pair"]]), int(b[h["pair"]])} == {int(sensors[k]), int(h["body"])}
        listed += len(hits)
    assert listed > 1000


def test_hand_made_cases():
    # records (0,1) (0,3) (1,2) (2,3); sensors 0 and 3; body 4 a sensor nobody touches
    a, b = [0, 0, 1, 2], [1, 3, 2, 3]
    sensors, offsets, hits = sm.occupancy(a, b, [1, 0, 0, 1, 1])
    assert sm.as_lists(sensors, offsets, hits) == [(0, [(1, 0), (3, 1)]), (3, [(0, 1), (2, 3)]), (4, [])]
    # nobody is a sensor / no records
    assert sm.as_lists(*sm.occupancy(a, b, [0] * 5)) == []
    assert sm.as_lists(*sm.occupancy([], [], [1, 1])) == [(0, []), (1, [])]


def test_the_record_is_the_bindings():
    assert capi.SENSOR_HIT_DTYPE == sm.HIT_DTYPE and sm.HIT_DTYPE.itemsize == 8
