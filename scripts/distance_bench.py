#!/usr/bin/env python3
"""Batched distance queries on the settled 262 144-box pile: one JSON line, also written to profiles/distance_bench.json.

  us_distance_grid / _brute  65 536 queries of a unit cube at a random pose inside the pile's box with max_distance = one cell edge: the
                             grid path, and the brute-force path on the first --brute-queries of them
  us_distance_points         65 536 point queries at the same positions, same max_distance, grid path
  us_overlap_grid, us_sweep_grid   the yardsticks: one overlap query call and one sweep call (along a random direction for one cell
                             edge) with the same volumes
  ratio_to_overlap / _points_to_overlap   us_distance_grid and us_distance_points over us_overlap_grid
  answers, overlaps          queries that find a body, and those that overlap one (both paths give the same bits for all queries; checked here)
  runs_us                    every timed call behind the medians
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

RUNS = {}


def timed(name, stream, call, repeats):
    """Median time in microseconds of `call` on `stream` after one warm-up call (scratch sized, code loaded); every run into RUNS."""
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
    RUNS[name] = times
    return statistics.median(times)


def distance_us(name, w, stream, q, flags, repeats):
    with torch.cuda.stream(stream):
        dev_q = torch.from_numpy(q.view(np.uint8).copy()).to("cuda")
        dev_hits = torch.empty(len(q) * 96, dtype=torch.uint8, device="cuda")
        t = timed(name, stream, lambda: w.distance_device(dev_q.data_ptr(), len(q), dev_hits.data_ptr(), flags), repeats)
        return t, dev_hits.cpu().numpy().view(capi.DISTANCE_HIT_DTYPE)


def sweep_us(w, stream, s, repeats):
    with torch.cuda.stream(stream):
        dev_s = torch.from_numpy(s.view(np.uint8).copy()).to("cuda")
        dev_hits = torch.empty(len(s) * 72, dtype=torch.uint8, device="cuda")
        return timed("sweep_grid", stream, lambda: w.sweep_device(dev_s.data_ptr(), len(s), dev_hits.data_ptr(), 0), repeats)


def overlap_us(w, stream, q, cap, repeats):
    with torch.cuda.stream(stream):
        dev_q = torch.from_numpy(q.view(np.uint8).copy()).to("cuda")
        dev_off = torch.zeros(len(q) + 1, dtype=torch.int32, device="cuda")
        dev_hits = torch.empty(max(cap, 1) * 16, dtype=torch.uint8, device="cuda")
        return timed("overlap_grid", stream, lambda: w.overlap_device(dev_q.data_ptr(), len(q), dev_off.data_ptr(), dev_hits.data_ptr(), cap, 0), repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--frames", type=int, default=120, help="frames the pile settles for")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--brute-queries", type=int, default=1024, help="queries the brute-force path is timed with (every query looks at every body)")
    ap.add_argument("--cells", type=float, default=1.0, help="max_distance in cell edges")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "distance_bench.json"))
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
    n = args.queries
    rot, d = rng.normal(size=(n, 4)), rng.normal(size=(n, 3))
    rot, d = rot / np.linalg.norm(rot, axis=1, keepdims=True), d / np.linalg.norm(d, axis=1, keepdims=True)
    pos = rng.uniform(lo, hi, (n, 3))
    reach = args.cells * edge
    q = capi.distances(pos, rot, 0, max_distance=reach)
    points = capi.distances(pos, max_distance=reach)

    t_grid, hits = distance_us("distance_grid", w, stream, q, 0, args.repeats)
    part = q[: args.brute_queries]
    t_brute, hits_b = distance_us("distance_brute", w, stream, part, capi.DISTANCE_BRUTE_FORCE, max(1, args.repeats // 3))
    t_points, hits_p = distance_us("distance_points", w, stream, points, 0, args.repeats)
    hits_all = w.distance(q, capi.DISTANCE_BRUTE_FORCE)  # not timed: the whole batch on the brute-force path, for the comparison
    volumes = capi.overlap_queries(pos, rot, 0)
    total = len(w.overlap(volumes)[1])
    t_overlap = overlap_us(w, stream, volumes, total, args.repeats)
    t_sweep = sweep_us(w, stream, capi.sweeps(pos, rot, d, 0, max_distance=reach), args.repeats)
    found, found_p = hits["body"] != capi.NO_HIT, hits_p["body"] != capi.NO_HIT
    res = {"bodies": args.bodies, "queries": n, "cells": args.cells, "cell_edge": edge, "brute_queries": len(part),
           "us_distance_grid": t_grid, "queries_per_s_grid": n / (t_grid * 1e-6),
           "us_distance_brute": t_brute, "queries_per_s_brute": len(part) / (t_brute * 1e-6),
           "us_distance_points": t_points, "points_per_s_grid": n / (t_points * 1e-6),
           "us_overlap_grid": t_overlap, "overlap_hits": total, "us_sweep_grid": t_sweep,
           "ratio_to_overlap": t_grid / t_overlap, "ratio_points_to_overlap": t_points / t_overlap,
           "answers": int(found.sum()), "overlaps": int((found & (hits["feature"] == capi.DISTANCE_OVERLAP)).sum()),
           "point_answers": int(found_p.sum()), "point_overlaps": int((found_p & (hits_p["feature"] == capi.DISTANCE_OVERLAP)).sum()),
           "same": bool(hits_b.tobytes() == hits[: len(part)].tobytes() and hits_all.tobytes() == hits.tobytes()),
           "runs_us": RUNS}
    w.set_stream(0)
    w.close()
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
