#!/usr/bin/env python3
"""Island sleeping on bench.py's two large contact scenes: one JSON line per scene, the whole result in --out.

  stacks  262 144 unit boxes in 16-high stacks (bench.py's stacks_262144_sat: SAT, 20 substeps): one island per stack
  pile    262 144 unit boxes dropped as a pile (4 layers at 1.8 m), pre-rolled to rest: ONE giant island of jittering boxes

Per scene, in this order:
  census        after the pre-roll, --census frames of a world WITHOUT sleeping: the largest linear / angular speed of every
                body over those frames, as percentiles.  The thresholds are set from it: --margin times the --percentile of those
                peaks (99.9 by default: a handful of bodies that never settle do not set the bar for everybody, and an island
                that holds one of them honestly never sleeps), unless given with --linear / --angular.
  ms_frame_off  one xpbd_world_step with the contact report on and sleeping off (HIP events on the world's stream, median of
                --repeats after --warmup)
  ms_frame_on_awake   the same frames with sleeping on and frames_to_sleep = UINT32_MAX: nothing ever sleeps, the difference to
                ms_frame_off is the cost of the pass, the records kernel and the inert test
  asleep        with frames_to_sleep = --frames-to-sleep: the fraction of bodies asleep after each of --run frames
  ms_frame_asleep     the median frame time of the last --repeats of those frames, next to the fraction asleep then
No speed-up is assumed anywhere: the numbers are what they are."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from constraint_solver_amd import capi  # noqa: E402

DT = 1.0 / 60.0
U32_MAX = 0xFFFFFFFF


def scene(name, n, seed):
    if name == "pile":
        kind = capi.SCENE_BOXES_DROP
        bodies, sid = capi.scene_pile(kind, seed, n, 1.8, 4)
        return kind, bodies, sid, bench.PREROLL_PILE
    kind = capi.SCENE_BOX_STACKS
    bodies, sid = capi.scene_generate(kind, seed, n, grid_w=bench.scene_grid_width(capi, kind, n, n))
    return kind, bodies, sid, bench.PREROLL["stacks"]


def timed(stream, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def world_of(kind, bodies, sid, stream):
    w = capi.World(mode=capi.MODE_CONTACTS)
    w.set_polytopes(capi.scene_polytopes(kind))
    w.set_narrowphase(capi.NARROWPHASE_SAT)
    w.upload(bodies, sid)
    w.set_stream(stream.cuda_stream)
    return w


def percentiles(v):
    return {"p50": float(np.percentile(v, 50)), "p99": float(np.percentile(v, 99)), "p999": float(np.percentile(v, 99.9)), "max": float(v.max())}


def run(name, args):
    kind, bodies, sid, preroll = scene(name, args.bodies, args.seed)
    preroll = args.preroll if args.preroll >= 0 else preroll
    n = len(bodies)
    stream = torch.cuda.current_stream()
    med = lambda v: statistics.median(v[-args.repeats:])
    out = {"scene": name, "bodies": n, "substeps": args.substeps, "preroll": preroll, "repeats": args.repeats, "warmup": args.warmup}
    with world_of(kind, bodies, sid, stream) as w:
        for _ in range(preroll):
            w.step(DT, args.substeps)
        w.set_contact_report(True)
        settled = w.download()                              # every later world starts from here
        # the census, and the frame without sleeping
        top_v, top_w = np.zeros(n), np.zeros(n)
        for _ in range(args.census):
            w.step(DT, args.substeps)
            s = w.download()
            top_v = np.maximum(top_v, np.linalg.norm(s[:, 22:25], axis=1))
            top_w = np.maximum(top_w, np.linalg.norm(s[:, 25:28], axis=1))
        out["census"] = {"frames": args.census, "linear": percentiles(top_v), "angular": percentiles(top_w)}
        off = [timed(stream, lambda: w.step(DT, args.substeps)) for _ in range(args.warmup + args.repeats)]
        out["ms_frame_off"] = med(off)
        out["broadphase_pairs_off"] = int(w.contact_stats()[0])
        w.set_stream(0)
    linear = args.linear if args.linear > 0 else args.margin * float(np.percentile(top_v, args.percentile))
    angular = args.angular if args.angular > 0 else args.margin * float(np.percentile(top_w, args.percentile))
    out["thresholds"] = {"linear_speed": linear, "angular_speed": angular, "frames_to_sleep": args.frames_to_sleep,
                         "from": "given" if args.linear > 0 else "%.2f x percentile %g of the census peaks" % (args.margin, args.percentile)}
    # sleeping on, nothing asleep: what the pass costs
    with world_of(kind, settled, sid, stream) as w:
        w.set_contact_report(True)
        w.set_sleeping(linear, angular, U32_MAX)
        awake = [timed(stream, lambda: w.step(DT, args.substeps)) for _ in range(args.census + args.warmup + args.repeats)]
        out["ms_frame_on_awake"] = med(awake)
        out["asleep_with_frames_to_sleep_max"] = w.sleep_state()[3][0]
        w.set_stream(0)
    # sleeping on
    with world_of(kind, settled, sid, stream) as w:
        w.set_contact_report(True)
        w.set_sleeping(linear, angular, args.frames_to_sleep)
        counts = torch.zeros(4, dtype=torch.int32, device="cuda")
        times, fraction = [], []
        for k in range(args.run):
            times.append(timed(stream, lambda: w.step(DT, args.substeps)))
            w.sleep_state_device(None, None, None, counts.data_ptr())
            fraction.append(int(counts.cpu().numpy().view(np.uint32)[0]) / n)
        out["asleep_fraction"] = {"frames": list(range(1, args.run + 1))[args.every - 1::args.every], "fraction": fraction[args.every - 1::args.every]}
        out["asleep_fraction_end"] = fraction[-1]
        out["sleeping_groups_end"] = int(counts.cpu().numpy().view(np.uint32)[1])
        out["ms_frame_asleep"] = med(times)
        out["broadphase_pairs_asleep"] = int(w.contact_stats()[0])
        w.set_stream(0)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="stacks,pile")
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--preroll", type=int, default=-1, help="frames before anything is measured (default: bench.py's for the scene)")
    ap.add_argument("--census", type=int, default=30)
    ap.add_argument("--margin", type=float, default=1.5)
    ap.add_argument("--percentile", type=float, default=99.9)
    ap.add_argument("--linear", type=float, default=0.0)
    ap.add_argument("--angular", type=float, default=0.0)
    ap.add_argument("--frames-to-sleep", type=int, default=30)
    ap.add_argument("--run", type=int, default=90)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    results = [run(name, args) for name in args.scenes.split(",")]
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"what": "scripts/sleeping_bench.py: a frame with sleeping off, on with nothing asleep, and on; HIP events on the world's "
                               "stream, median of the last %d frames" % args.repeats, "scenes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
