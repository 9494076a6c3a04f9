#!/usr/bin/env python3
"""Batched sweep queries on the settled 262 144-box pile: one JSON line, also written to profiles/sweep_bench.json.

  us_sweep_grid / _brute     65 536 sweeps of a unit cube at a random pose inside the pile's box, along a random direction for about
                             four cell edges: the grid path, and the brute-force path on the first --brute-sweeps of them
  sweeps_per_s_grid / _brute the same as rates
  us_overlap_grid            the yardstick: one overlap query call with the same volumes at their start poses
  hits, initial              sweeps that hit something, and those that start in overlap (both paths give the same bits for all sweeps; checked here)
Device times are the median of --repeats stream-ordered calls of the device variant, timed with HIP events on the world's stream
after a warm-up call."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch  # first: the library then binds to the HIP runtime torch carries

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from constraint_solver_amd import capi  # noqa: E402


def timed(stream, call, repeats):
    """Median time in microseconds of `call` on `stream` after one warm-up call (scratch sized, code loaded)."""
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
    return statistics.median(times)


def sweep_us(w, stream, s, flags, repeats):
    with torch.cuda.stream(stream):
        dev_s = torch.from_numpy(s.view(np.uint8).copy()).to("cuda")
        dev_hits = torch.empty(len(s) * 72, dtype=torch.uint8, device="cuda")
        t = timed(stream, lambda: w.sweep_device(dev_s.data_ptr(), len(s), dev_hits.data_ptr(), flags), repeats)
        return t, dev_hits.cpu().numpy().view(capi.SWEEP_HIT_DTYPE)


def overlap_us(w, stream, q, cap, repeats):
    with torch.cuda.stream(stream):
        dev_q = torch.from_numpy(q.view(np.uint8).copy()).to("cuda")
        dev_off = torch.zeros(len(q) + 1, dtype=torch.int32, device="cuda")
        dev_hits = torch.empty(max(cap, 1) * 16, dtype=torch.uint8, device="cuda")
        return timed(stream, lambda: w.overlap_device(dev_q.data_ptr(), len(q), dev_off.data_ptr(), dev_hits.data_ptr(), cap, 0), repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--frames", type=int, default=120, help="frames the pile settles for")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--sweeps", type=int, default=65536)
    ap.add_argument("--brute-sweeps", type=int, default=1024, help="sweeps the brute-force path is timed with (every sweep looks at every body)")
    ap.add_argument("--cells", type=float, default=4.0, help="length of a sweep in cell edges")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sweep_bench.json"))
    args = ap.parse_args()

    bodies, sid = capi.scene_pile(capi.SCENE_BOXES_DROP, args.seed, args.bodies, 2.0, 4)
    cube = capi.polytope(capi.SHAPE_CUBE)
    w = capi.World(mode=capi.MODE_CONTACTS)
    w.set_polytopes([cube])
    w.upload(bodies, sid)
    for _ in range(args.frames):
        w.step(1.0 / 60.0, 20)
    state = w.download()
    stream = torch.cuda.Stream()                      # not the null stream: the world's work and the events share one queue
    w.set_stream(stream.cuda_stream)

    rng = np.random.default_rng(args.seed)
    centre = state[:, 31:34] + state[:, 28:31]
    lo, hi = centre.min(axis=0), centre.max(axis=0)
    v = np.asarray(cube["vertices"], dtype=np.float64).reshape(-1, 3)
    edge = 2.0 * float(np.linalg.norm(v - np.asarray(cube["centroid"]), axis=1).max()) * (1.0 + 1e-6)   # the grid's cell edge
    n = args.sweeps
    rot, d = rng.normal(size=(n, 4)), rng.normal(size=(n, 3))
    rot, d = rot / np.linalg.norm(rot, axis=1, keepdims=True), d / np.linalg.norm(d, axis=1, keepdims=True)
    pos = rng.uniform(lo, hi, (n, 3))
    s = capi.sweeps(pos, rot, d, 0, max_distance=args.cells * edge)
    q = capi.overlap_queries(pos, rot, 0)

    t_grid, hits = sweep_us(w, stream, s, 0, args.repeats)
    part = s[: args.brute_sweeps]
    t_brute, hits_b = sweep_us(w, stream, part, capi.SWEEP_BRUTE_FORCE, max(1, args.repeats // 3))
    hits_all = w.sweep(s, capi.SWEEP_BRUTE_FORCE)     # not timed: the whole batch on the brute-force path, for the comparison
    total = len(w.overlap(q)[1])
    t_overlap = overlap_us(w, stream, q, total, args.repeats)
    found = hits["body"] != capi.NO_HIT
    res = {"bodies": args.bodies, "sweeps": n, "cells": args.cells, "cell_edge": edge, "brute_sweeps": len(part),
           "us_sweep_grid": t_grid, "sweeps_per_s_grid": n / (t_grid * 1e-6),
           "us_sweep_brute": t_brute, "sweeps_per_s_brute": len(part) / (t_brute * 1e-6),
           "us_overlap_grid": t_overlap, "overlap_hits": total,
           "hits": int(found.sum()), "initial": int((found & (hits["feature"] == capi.SWEEP_INITIAL)).sum()),
           "same": bool(hits_b.tobytes() == hits[: len(part)].tobytes() and hits_all.tobytes() == hits.tobytes())}
    w.set_stream(0)
    w.close()
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
