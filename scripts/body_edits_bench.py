#!/usr/bin/env python3
"""Body edits on bench.py's boxes pile (262 144 unit boxes, XPBD_MODE_CONTACTS): one JSON line.

  wrench_device_us     xpbd_world_set_external_wrench_device for ALL bodies (indices == NULL, force and torque)
  impulses_device_us   xpbd_world_apply_impulses_device with one entry per body (at a point, with an angular impulse)
  upload_bodies_us     what a host had to do for the same effect before the edits existed: xpbd_world_upload_bodies of the whole
                       array (it waits, so the events bracket the whole call)
  frame_us             one xpbd_world_step(1/60, 20) of the pile, the yardstick the edits are stated against
Every figure is the median of --repeats calls after --warmup, timed with HIP events on the world's stream (a torch stream
handed over with set_stream).  GB/s = the bytes the kernel has to move (wrench: 48 read + 48 written per body; impulses: 80
read per entry + 22 doubles read and 6 written per body) over the time, next to the device-to-device copy roof
(xpbd_selftest_hbm_copy).  Recorded, not gated."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch  # first: the library then binds to the HIP runtime torch carries

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from constraint_solver_amd import capi  # noqa: E402


def median_us(stream, call, warmup, repeats):
    for _ in range(warmup):
        call()
    stream.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(stream)
        call()
        b.record(stream)
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e3)
    return statistics.median(times), min(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--preroll", type=int, default=30, help="frames the pile runs before anything is timed")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    args = ap.parse_args()
    n, kind = args.bodies, capi.SCENE_BOXES_DROP
    bodies, sid = capi.scene_pile(kind, args.seed, n, 1.8, 4)
    rng = np.random.default_rng(args.seed)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream), capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(kind))
        w.upload(bodies, sid)
        w.set_stream(stream.cuda_stream)
        for _ in range(args.preroll):
            w.step(1.0 / 60.0, 20)
        state = w.download()
        frame_us, frame_min = median_us(stream, lambda: w.step(1.0 / 60.0, 20), 2, args.repeats)

        force = torch.from_numpy(rng.normal(0.0, 1.0, (n, 3))).to("cuda")
        torque = torch.from_numpy(rng.normal(0.0, 0.1, (n, 3))).to("cuda")
        wrench_us, wrench_min = median_us(stream, lambda: w.set_external_wrench_device(0, n, force.data_ptr(), torque.data_ptr()),
                                          args.warmup, args.repeats)
        entries = capi.impulses(np.arange(n), rng.normal(0.0, 0.01, (n, 3)), point=state[:, 31:34] + state[:, 28:31] + 0.1,
                                angular_impulse=rng.normal(0.0, 0.001, (n, 3)))
        dev_entries = torch.from_numpy(entries.view(np.uint8).copy()).to("cuda")
        impulses_us, impulses_min = median_us(stream, lambda: w.apply_impulses_device(dev_entries.data_ptr(), n), args.warmup, args.repeats)
        edited = w.download()
        upload_us, upload_min = median_us(stream, lambda: w.upload(edited, sid), args.warmup, args.repeats)
        w.set_stream(0)
    roof = capi.selftest_hbm_copy()
    wrench_bytes, impulse_bytes = n * 96, n * (80 + 22 * 8 + 6 * 8)
    result = {"bodies": n, "repeats": args.repeats, "frame_us": frame_us, "frame_us_min": frame_min,
              "wrench_device_us": wrench_us, "wrench_device_us_min": wrench_min, "wrench_fraction_of_frame": wrench_us / frame_us,
              "wrench_gbytes_per_s": wrench_bytes / (wrench_us * 1e3),
              "impulses_device_us": impulses_us, "impulses_device_us_min": impulses_min, "impulses_fraction_of_frame": impulses_us / frame_us,
              "impulses_gbytes_per_s": impulse_bytes / (impulses_us * 1e3),
              "upload_bodies_us": upload_us, "upload_bodies_us_min": upload_min, "upload_fraction_of_frame": upload_us / frame_us,
              "hbm_copy_gbytes_per_s": roof, "finite": bool(np.isfinite(edited).all())}
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
