#!/usr/bin/env python3
"""Restitution on bench.py's piles (SAT, 20 substeps): one JSON line per run, in the manner of material_bench.py.

  --scene boxes   262 144 unit boxes in 4 layers at 1.8 m
  --scene mixed   65 536 mixed polyhedra in 4 layers at 1.4 m
The pile is pre-rolled without restitution into its resting regime; then --config is set, a few frames warm up, and --frames
frames are timed (wall time per frame, the world synchronised).
  none   no xpbd_world_set_restitution call: the fused schedule, the kernels of a world before restitution
  zero   every coefficient 0: must be `none` (same schedule, same checksum)
  half   every body and the ground 0.5: the unfused schedule plus the velocity pass
XPBD_HIP_LIB=<another libxpbd_hip.so> runs an older build (--config none only): the A/B of the unchanged path.  Run the two
builds alternately in one call, and the older one against itself: that spread is the yardstick."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from constraint_solver_amd import capi  # noqa: E402

SCENES = {"boxes": (capi.SCENE_BOXES_DROP, 262144, 1.8), "mixed": (capi.SCENE_MIXED_DROP, 65536, 1.4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=sorted(SCENES), default="boxes")
    ap.add_argument("--config", choices=["none", "zero", "half"], default="none")
    ap.add_argument("--bodies", type=int, default=0)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--preroll", type=int, default=180)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    kind, n, pitch = SCENES[args.scene]
    n = args.bodies or n
    dt = 1.0 / 60.0
    bodies, sid = capi.scene_pile(kind, args.seed, n, pitch, 4)
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(kind))
        w.set_narrowphase(capi.NARROWPHASE_SAT)
        w.upload(bodies, sid)
        for _ in range(args.preroll):
            w.step(dt, args.substeps)
        if args.config != "none":
            e = 0.5 if args.config == "half" else 0.0
            w.set_restitution(np.full(n, e), e, 0.0)
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
        state = w.download()
    median = statistics.median(times)
    print(json.dumps({"scene": args.scene, "config": args.config, "lib": os.environ.get("XPBD_HIP_LIB", "built"), "bodies": n,
                      "substeps": args.substeps, "frames": args.frames, "ms_per_frame_median": 1e3 * median,
                      "ms_per_frame_min": 1e3 * min(times), "body_substeps_per_s": n * args.substeps / median, "pairs": pairs,
                      "touching_per_substep": touching / (args.frames * args.substeps),
                      "points_per_substep": points / (args.frames * args.substeps), "finite": bool(np.isfinite(state).all()),
                      "state_crc": int(np.bitwise_xor.reduce(state.view(np.uint64).ravel()))}))


if __name__ == "__main__":
    main()
