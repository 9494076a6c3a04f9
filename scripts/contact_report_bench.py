#!/usr/bin/env python3
"""Contact reports on bench.py's boxes pile (262 144 unit boxes in 4 layers at 1.8 m, SAT, 20 substeps): one JSON line.

The pile is pre-rolled with reporting off (bench.py's PREROLL_PILE frames) into its resting regime; then --config is applied,
a few frames warm up, and --frames frames are timed (wall time per frame, the world synchronised).
  off       reporting off (no report kernel runs)
  counts    reporting on, xpbd_world_contact_report_counts every frame (touch counts, key compaction, scans, event flags)
  download  reporting on, counts + every pair record, point and event downloaded every frame (ms_download: that part alone)
Kernel times come from a run under `rocprofv3 --kernel-trace --stats` (k_report_*)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from constraint_solver_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["off", "counts", "download"], default="off")
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
        if args.config != "off":
            w.set_contact_report(True)
        for _ in range(args.warmup):
            w.step(dt, args.substeps)
        w.synchronize()
        w.contact_stats()                                  # resets the per-substep sums
        times, step_times, download_times, counts = [], [], [], None
        for _ in range(args.frames):
            t0 = time.perf_counter()
            w.step(dt, args.substeps)
            w.synchronize()
            t1 = time.perf_counter()
            if args.config != "off":
                counts = w.contact_report_counts()
            t2 = time.perf_counter()
            if args.config == "download":
                w.pair_contacts()
                w.contact_events()
            t3 = time.perf_counter()
            times.append(t3 - t0)
            step_times.append(t1 - t0)
            download_times.append(t3 - t2)
        pairs, touching, points = w.contact_stats()
    print(json.dumps({"config": args.config, "bodies": args.bodies, "substeps": args.substeps, "frames": args.frames,
                      "ms_per_frame_median": 1e3 * statistics.median(times), "ms_per_frame_min": 1e3 * min(times),
                      "ms_step_median": 1e3 * statistics.median(step_times), "ms_download_median": 1e3 * statistics.median(download_times),
                      "pairs": pairs, "touching_per_substep": touching / (args.frames * args.substeps),
                      "points_per_substep": points / (args.frames * args.substeps),
                      "report_counts": counts}))


if __name__ == "__main__":
    main()
