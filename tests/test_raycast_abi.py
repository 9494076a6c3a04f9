"""The ray-cast ABI without a device: record layouts and argument errors that are caught before any device work."""
import ctypes as C

import numpy as np

from constraint_solver_amd import capi


def test_ray_records_are_64_bytes():
    assert capi.RAY_DTYPE.itemsize == 64 and capi.RAY_HIT_DTYPE.itemsize == 64
    assert capi.RAY_DTYPE.fields["max_distance"][1] == 48 and capi.RAY_DTYPE.fields["ignore_body"][1] == 56
    assert capi.RAY_HIT_DTYPE.fields["distance"][1] == 8 and capi.RAY_HIT_DTYPE.fields["normal"][1] == 40


def test_rays_helper_broadcasts_and_defaults():
    r = capi.rays([[0.0, 0.0, 5.0]], [[0.0, 0.0, -1.0], [1.0, 0.0, 0.0]], max_distance=3.0, ignore=[4, 7])
    assert r.shape == (2,) and (r["origin"][:, 2] == 5.0).all() and (r["max_distance"] == 3.0).all()
    assert list(r["ignore_body"]) == [4, 7] and (r["reserved"] == 0).all()
    assert (capi.rays(np.zeros((3, 3)), [1.0, 0.0, 0.0])["ignore_body"] == capi.NO_HIT).all()


def test_null_world_buffers_and_unknown_flags_are_invalid():
    L = capi.hip_lib()
    rays = capi.rays([[0.0, 0.0, 0.0]], [[1.0, 0.0, 0.0]])
    hits = np.zeros(1, dtype=capi.RAY_HIT_DTYPE)
    for fn in (L.xpbd_world_raycast, L.xpbd_world_raycast_device, L.xpbd_multi_world_raycast):
        assert fn(None, rays.ctypes.data, 1, 0, hits.ctypes.data) == capi.E_INVALID
        assert b"NULL" in L.xpbd_last_error()
        assert fn(None, None, 0, 0, None) == capi.E_INVALID
    # a handle is needed to get past the NULL-world check; without a device none can be made, so the remaining checks
    # (NULL buffers, flags, reserved) run on the GPU (tests/test_gpu_raycast.py)
    assert hits["body"][0] == 0
