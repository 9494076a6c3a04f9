#!/usr/bin/env python3
"""Collision filters on bench.py's boxes pile (262 144 unit boxes in 4 layers at 1.8 m, SAT, 20 substeps): one JSON line.

The pile is pre-rolled without filters (bench.py's PREROLL_PILE frames) into its resting regime; then the filters of
--config are set, a few frames warm up, and --frames frames are timed (wall time per frame, the world synchronised).
  none   no filters (the plain neighbour kernels)
  ones   every body {~0, ~0}: the filtered neighbour kernels, nothing filtered
  half   the odd bodies {2, 1}, the even ones {1, 3}: odd bodies do not collide with each other
Kernel times come from a run under `rocprofv3 --kernel-trace --stats` (k_neighbour_count, k_neighbour_fill, the SAT
kernels).  XPBD_HIP_LIB=<another libxpbd_hip.so> runs an older build (--config none only): the A/B of the plain kernels."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from constraint_solver_amd import capi  # noqa: E402

ALL = 0xFFFFFFFF


def filters_for(config, n):
    if config == "none":
        return None
    f = np.zeros(n, dtype=capi.COLLISION_FILTER_DTYPE)
    if config == "ones":
        f["group"], f["mask"] = ALL, ALL
    else:
        f["group"][0::2], f["mask"][0::2] = 1, 3
        f["group"][1::2], f["mask"][1::2] = 2, 1
    return f


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["none", "ones", "half"], default="none")
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--preroll", type=int, default=180)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    dt = 1.0 / 60.0
    bodies, sid = capi.scene_pile(capi.SCENE_BOXES_DROP, args.seed, args.bodies, 1.8, 4)
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES_DROP))
        w.set_narrowphase(capi.NARROWPHASE_SAT)
        w.upload(bodies, sid)
        for _ in range(args.preroll):
            w.step(dt, args.substeps)
        f = filters_for(args.config, args.bodies)
        if f is not None:
            w.set_collision_filters(f)
        for _ in range(args.warmup):
            w.step(dt, args.substeps)
        w.synchronize()
        w.contact_stats()                                  # resets the per-substep sums
        times = []
        for _ in range(args.frames):
            t0 = time.perf_counter()
            w.step(dt, args.substeps)
            w.synchronize()
            times.append(time.perf_counter() - t0)
        pairs, touching, points = w.contact_stats()
    print(json.dumps({"config": args.config, "lib": os.environ.get("XPBD_HIP_LIB", "built"), "bodies": args.bodies,
                      "substeps": args.substeps, "frames": args.frames, "ms_per_frame_median": 1e3 * statistics.median(times),
                      "ms_per_frame_min": 1e3 * min(times), "pairs": pairs, "touching_per_substep": touching / (args.frames * args.substeps),
                      "points_per_substep": points / (args.frames * args.substeps)}))


if __name__ == "__main__":
    main()
