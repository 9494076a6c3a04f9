"""Child process of tests/test_gpu_terrain_distance.py: the device variant of the terrain distance queries, with torch tensors on a
torch stream handed to the world with set_stream.  torch is imported first, so that the library binds to the HIP runtime torch
carries (as in bench.py).  Prints one JSON line of verdicts."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from constraint_solver_amd import capi  # noqa: E402
import test_gpu_terrain_distance as t  # noqa: E402

GUARD = 16
SIZE = 96


def main():
    torch.cuda.set_device(0)
    polys = capi.scene_polytopes(t.MIXED)
    w = t.world(t.RECIPE, polys)
    q = t.recipe_queries(np.random.default_rng(7), 1025, t.RECIPE, len(polys))
    host = w.terrain_distance(q)
    res = {"terrain_seen": bool((host["body"] == capi.HIT_TERRAIN).sum() > 400 and (host["body"] == capi.NO_HIT).sum() > 100)}
    stream = torch.cuda.Stream()
    w.set_stream(stream.cuda_stream)
    guard = True

    def records(flags):
        """The device call on tensors of the queries and of len(q) + GUARD records; the raw bytes back."""
        nonlocal guard
        dev_in = torch.from_numpy(q.view(np.uint8).copy()).to("cuda")
        dev_out = torch.full(((len(q) + GUARD) * SIZE,), 0xEE, dtype=torch.uint8, device="cuda")
        w.terrain_distance_device(dev_in.data_ptr(), len(q), dev_out.data_ptr(), flags)
        raw = dev_out.cpu().numpy()                             # (the copy is ordered after the query on the same stream)
        guard = guard and bool((raw[len(q) * SIZE:] == 0xEE).all())
        return raw[:len(q) * SIZE].tobytes()

    with torch.cuda.stream(stream):
        res["walk"] = records(0) == host.tobytes()
        res["brute"] = records(t.BRUTE) == host.tobytes()
        res["masked"] = records(t.MASKED) == host.tobytes()
        w.set_terrain(None)
        dev_out = torch.full((SIZE,), 0xEE, dtype=torch.uint8, device="cuda")
        rc = capi.hip_lib().xpbd_world_terrain_distance_device(w._h, dev_out.data_ptr(), 1, 0, dev_out.data_ptr())
        res["no_terrain_is_invalid"] = rc == capi.E_INVALID and bool((dev_out.cpu().numpy() == 0xEE).all())
        res["guard"] = guard
    w.set_stream(0)
    w.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
