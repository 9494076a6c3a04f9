#!/usr/bin/env python3
"""Batched ray casts on the settled 262 144-box pile: one JSON line.

  rays_per_s_random   1 048 576 random rays inside the pile's box (device variant, grid path: build + traversal)
  rays_per_s_fan      a 1024 x 1024 camera fan from above
  grid_build_us       the grid path with 9 rays (build + a negligible traversal)
  traversal_us_*      the 1M-ray time minus grid_build_us
  brute_us_1 / _64    the brute-force path for 1 and 64 rays
  pick_wall_us        wall time of one host-variant xpbd_world_raycast with a single ray (picking latency)
Device times are the median of --repeats stream-ordered calls timed with HIP events."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # first: the library then binds to the HIP runtime torch carries

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from constraint_solver_amd import capi  # noqa: E402


def device_us(w, stream, r, flags, repeats):
    """Median time of the device variant on `stream` (the world's stream), HIP events recorded on that stream."""
    with torch.cuda.stream(stream):
        dev_rays = torch.from_numpy(r.view(np.uint8).copy()).to("cuda")
        dev_hits = torch.empty(len(r) * 64, dtype=torch.uint8, device="cuda")
        w.raycast_device(dev_rays.data_ptr(), len(r), dev_hits.data_ptr(), flags)   # scratch sized, code loaded
        stream.synchronize()
        times = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            w.raycast_device(dev_rays.data_ptr(), len(r), dev_hits.data_ptr(), flags)
            b.record(stream)
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        hits = dev_hits.cpu().numpy().view(capi.RAY_HIT_DTYPE)
    return statistics.median(times), hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--frames", type=int, default=120, help="frames the pile settles for")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    bodies, sid = capi.scene_pile(capi.SCENE_BOXES_DROP, args.seed, args.bodies, 2.0, 4)
    w = capi.World(mode=capi.MODE_CONTACTS)
    w.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES_DROP))
    w.upload(bodies, sid)
    for _ in range(args.frames):
        w.step(1.0 / 60.0, 20)
    state = w.download()
    stream = torch.cuda.Stream()                      # not the null stream: the world's work and the events share one queue
    w.set_stream(stream.cuda_stream)

    rng = np.random.default_rng(args.seed)
    centre = state[:, 31:34] + state[:, 28:31]
    lo, hi = centre.min(axis=0), centre.max(axis=0)
    n = 1 << 20
    d = rng.normal(size=(n, 3))
    random_rays = capi.rays(rng.uniform(lo, hi, size=(n, 3)), d / np.linalg.norm(d, axis=1, keepdims=True))
    side = 1024
    u, v = np.meshgrid(np.linspace(lo[0], hi[0], side), np.linspace(lo[1], hi[1], side))
    eye = np.array([0.5 * (lo[0] + hi[0]), 0.5 * (lo[1] + hi[1]), hi[2] + 50.0])
    targets = np.stack([u.ravel(), v.ravel(), np.full(side * side, lo[2])], axis=1)
    fan = capi.rays(np.broadcast_to(eye, targets.shape), targets - eye)

    t_random, h_random = device_us(w, stream, random_rays, 0, args.repeats)
    t_fan, h_fan = device_us(w, stream, fan, 0, args.repeats)
    t_build, _ = device_us(w, stream, random_rays[:9], 0, args.repeats)
    t_b1, _ = device_us(w, stream, random_rays[:1], capi.RAYCAST_BRUTE_FORCE, args.repeats)
    t_b64, _ = device_us(w, stream, random_rays[:64], capi.RAYCAST_BRUTE_FORCE, args.repeats)
    torch.cuda.synchronize()
    one = fan[side * side // 2 + side // 2: side * side // 2 + side // 2 + 1]
    w.raycast(one)
    walls = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        w.raycast(one)
        walls.append((time.perf_counter() - t0) * 1e6)
    w.set_stream(0)
    w.close()
    print(json.dumps({
        "bodies": args.bodies, "rays_random": n, "rays_fan": side * side,
        "rays_per_s_random": n / (t_random * 1e-6), "rays_per_s_fan": side * side / (t_fan * 1e-6),
        "us_random": t_random, "us_fan": t_fan, "grid_build_us": t_build,
        "traversal_us_random": t_random - t_build, "traversal_us_fan": t_fan - t_build,
        "brute_us_1": t_b1, "brute_us_64": t_b64, "pick_wall_us": statistics.median(walls),
        "hit_fraction_random": float(np.mean(h_random["body"] != capi.NO_HIT)),
        "hit_fraction_fan": float(np.mean(h_fan["body"] != capi.NO_HIT)),
    }))


if __name__ == "__main__":
    main()
