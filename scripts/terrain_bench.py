#!/usr/bin/env python3
"""What a heightfield terrain costs (SAT, 20 substeps): 262 144 unit boxes in 4 layers at 1.8 m, settled on their ground, in
three worlds that are timed in turn, round after round, in one process:

  plane_fused     the plane z = 0, no terrain: the fused schedule, the kernels of a world before terrain
  plane_unfused   the plane z = 0 forced onto the unfused schedule by a restitution that never fires
                  (ground_restitution = 1e-300): one kernel sequence per substep plus the velocity pass
  terrain         a rolling field A sin(2 pi x / L) sin(2 pi y / L), L = 4 m, eight samples per wavelength, every body lifted
                  by the height under its centre plus A: the unfused schedule with the lookup in its ground stage

plane_unfused - plane_fused is the price of the schedule, terrain - plane_unfused that of the lookup (the velocity pass of
plane_unfused, which terrain alone does not run, counts against the schedule here).  Each world is pre-rolled into its resting
regime; then `--rounds` times each world steps `--frames` frames (wall time per frame, the world synchronised).  One JSON
object; --out also writes it to a file."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from constraint_solver_amd import capi  # noqa: E402

CONFIGS = ("plane_fused", "plane_unfused", "terrain")


def rolling_field(bodies, amplitude, wavelength):
    """(heights, origin, cell) of the field under the bodies' footprint and two wavelengths around it."""
    cell = wavelength / 8.0
    margin = 2.0 * wavelength + 2.0
    lo = bodies[:, 31:33].min(axis=0) - margin
    hi = bodies[:, 31:33].max(axis=0) + margin
    nx, ny = (int(math.ceil((hi[a] - lo[a]) / cell)) + 1 for a in (0, 1))
    if nx * ny > capi.MAX_TERRAIN_SAMPLES:
        raise SystemExit("the field needs %d x %d samples: more than the cap" % (nx, ny))
    k = 2.0 * math.pi / wavelength
    x, y = lo[0] + cell * np.arange(nx), lo[1] + cell * np.arange(ny)
    return amplitude * np.sin(k * y)[:, None] * np.sin(k * x)[None, :], (float(lo[0]), float(lo[1])), (cell, cell)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--amplitude", type=float, default=0.3)
    ap.add_argument("--wavelength", type=float, default=4.0)
    ap.add_argument("--preroll", type=int, default=180)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    kind, n, dt = capi.SCENE_BOXES_DROP, args.bodies, 1.0 / 60.0
    bodies, sid = capi.scene_pile(kind, args.seed, n, 1.8, 4)
    heights, origin, cell = rolling_field(bodies, args.amplitude, args.wavelength)
    worlds, result = {}, {"bodies": n, "substeps": args.substeps, "frames_per_round": args.frames, "rounds": args.rounds,
                          "field": {"samples": [heights.shape[1], heights.shape[0]], "cell": cell[0], "amplitude": args.amplitude,
                                    "wavelength": args.wavelength, "plane_table_MiB": (heights.shape[0] - 1) * (heights.shape[1] - 1) * 64 / 2.0**20}}
    try:
        for name in CONFIGS:
            w = worlds[name] = capi.World(mode=capi.MODE_CONTACTS)
            w.set_polytopes(capi.scene_polytopes(kind))
            w.set_narrowphase(capi.NARROWPHASE_SAT)
            start = bodies
            if name == "terrain":
                t0 = time.perf_counter()
                w.set_terrain(heights, origin, cell)
                result["set_terrain_ms"] = 1e3 * (time.perf_counter() - t0)
                start = bodies.copy()
                start[:, 33] += w.sample_terrain(bodies[:, 31:33] + bodies[:, 28:30], normals=False) + abs(args.amplitude)
            w.upload(start, sid)
            if name == "plane_unfused":
                w.set_restitution(None, 1e-300, 0.0)
            for _ in range(args.preroll + args.warmup):
                w.step(dt, args.substeps)
            w.synchronize()
            w.contact_stats()                                  # resets the per-substep sums
        times = {name: [] for name in CONFIGS}
        for _ in range(args.rounds):
            for name in CONFIGS:
                w = worlds[name]
                for _ in range(args.frames):
                    t0 = time.perf_counter()
                    w.step(dt, args.substeps)
                    w.synchronize()
                    times[name].append(time.perf_counter() - t0)
        for name in CONFIGS:
            w = worlds[name]
            pairs, touching, points = w.contact_stats()
            state = w.download()
            per_round = [statistics.median(times[name][r * args.frames:(r + 1) * args.frames]) for r in range(args.rounds)]
            median = statistics.median(times[name])
            result[name] = {"ms_per_frame_median": 1e3 * median, "ms_per_frame_min": 1e3 * min(times[name]),
                            "ms_per_frame_round_medians": [1e3 * t for t in per_round], "body_substeps_per_s": n * args.substeps / median,
                            "ground_contacts_last_substep": int(len(w.contacts())), "pairs": pairs,
                            "touching_per_substep": touching / (args.rounds * args.frames * args.substeps),
                            "finite": bool(np.isfinite(state).all()), "lowest_z": float(state[:, 33].min())}
            if name == "terrain":                               # who left the field, and how the others stand on it
                centre = state[:, 31:34] + state[:, 28:31]
                ground = w.sample_terrain(centre[:, :2], normals=False)
                over = ~np.isnan(ground)
                result[name].update({"centres_beyond_the_field": int((~over).sum()), "lowest_z_over_the_field": float(state[over, 33].min()),
                                     "lowest_centre_above_ground": float((centre[over, 2] - ground[over]).min())})
    finally:
        for w in worlds.values():
            w.close()
    fused, unfused, terrain = (result[name]["ms_per_frame_median"] for name in CONFIGS)
    result["schedule_ms_per_frame"] = unfused - fused
    result["lookup_ms_per_frame"] = terrain - unfused
    text = json.dumps(result)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
