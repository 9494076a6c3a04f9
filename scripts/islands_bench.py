#!/usr/bin/env python3
"""Contact islands on bench.py's two large scenes: one JSON line per scene, the whole result in --out.

  pile    262 144 unit boxes dropped as a pile (4 layers at 1.8 m, SAT, 20 substeps), pre-rolled to rest: ONE giant island,
          the contention worst case of the records' atomics
  joints  262 144 unit boxes at 2 m with 65 408 joints in chains of five: many small islands

Per scene, HIP events on the world's stream, median of --repeats after --warmup:
  ms_frame            one xpbd_world_step of the scene (reports on)
  ms_islands_frame    xpbd_world_islands_device as the first report consumer of a frame (it compacts the frame's keys)
  ms_islands_repeat   the same call again in the same frame (keys ready: the islands pass alone)
and, wall time with the world synchronised, what a host needed before for the same answer:
  ms_host_download    xpbd_world_download_pair_contacts (records only) + xpbd_world_download_bodies
(the union-find on the host comes on top of that and is not timed).  Kernel times: run under `rocprofv3 --kernel-trace --stats`
(k_islands_*), in a run of its own."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from constraint_solver_amd import capi  # noqa: E402

DT = 1.0 / 60.0


def scene(name, n, seed):
    kind = capi.SCENE_BOXES_DROP
    if name == "pile":
        bodies, sid = capi.scene_pile(kind, seed, n, 1.8, 4)
        return bodies, sid, None, bench.PREROLL_PILE
    grid_w = bench.scene_grid_width(capi, kind, n, n)
    bodies, sid = capi.scene_generate(kind, seed, n, grid_w=grid_w)
    joints = bench.chain_joints(capi, np, n // 4, n, 2.0, grid_w, state=bodies)
    return bodies, sid, joints, bench.PREROLL["boxes-drop"]


def timed(stream, call):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    call()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def run(name, args):
    bodies, sid, joints, preroll = scene(name, args.bodies, args.seed)
    n = len(bodies)
    stream = torch.cuda.current_stream()
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(capi.SCENE_BOXES_DROP))
        w.set_narrowphase(capi.NARROWPHASE_SAT)
        w.upload(bodies, sid)
        if joints is not None:
            w.set_joints(joints)
        w.set_stream(stream.cuda_stream)
        for _ in range(args.preroll if args.preroll >= 0 else preroll):
            w.step(DT, args.substeps)
        w.set_contact_report(True)
        island_of = torch.zeros(n, dtype=torch.int32, device="cuda")
        records = torch.zeros(n * capi.ISLAND_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
        total = torch.zeros(1, dtype=torch.int32, device="cuda")
        call = lambda: w.islands_device(0, island_of.data_ptr(), records.data_ptr(), n, total.data_ptr())
        frame, first, repeat, host = [], [], [], []
        for k in range(args.warmup + args.repeats):
            frame.append(timed(stream, lambda: w.step(DT, args.substeps)))
            first.append(timed(stream, call))
        for k in range(args.warmup + args.repeats):
            repeat.append(timed(stream, call))
        for k in range(args.warmup + args.repeats):
            w.step(DT, args.substeps)
            w.synchronize()
            t0 = time.perf_counter()
            pairs, _ = w.pair_contacts(points=False)
            w.download()
            host.append(1e3 * (time.perf_counter() - t0))
        call()                                             # the last frame once more, for the comparison with the host call
        host_of, host_records = w.islands(0)
        same = (int(total.cpu().numpy().view(np.uint32)[0]) == len(host_records)
                and np.array_equal(island_of.cpu().numpy().view(np.uint32), host_of)
                and records.cpu().numpy()[:host_records.nbytes].tobytes() == host_records.tobytes())
        w.set_stream(0)
    med = lambda v: statistics.median(v[args.warmup:])
    out = {"scene": name, "bodies": n, "joints": 0 if joints is None else int(len(joints)), "substeps": args.substeps,
           "touching_pairs": int(len(pairs)), "islands": int(len(host_records)), "largest_island": int(host_records["n_bodies"].max()),
           "device_call_equals_host_call": bool(same),
           "ms_frame": med(frame), "ms_islands_frame": med(first), "ms_islands_repeat": med(repeat), "ms_host_download": med(host),
           "repeats": args.repeats, "warmup": args.warmup}
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", default="pile,joints")
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--preroll", type=int, default=-1, help="frames before anything is timed (default: bench.py's for the scene)")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    results = [run(name, args) for name in args.scenes.split(",")]
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"what": "scripts/islands_bench.py: xpbd_world_islands_device against one frame and against the downloads a host "
                               "needed before; HIP events on the world's stream, median of %d after %d" % (args.repeats, args.warmup),
                       "scenes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
