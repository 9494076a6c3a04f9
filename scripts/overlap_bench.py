#!/usr/bin/env python3
"""Batched overlap queries on the settled 262 144-box pile: one JSON line.

  us_small_grid / _brute   65 536 body-sized queries (a unit cube at a random pose inside the pile's box): the grid path and the
                           brute-force path of this build, its reference point
  us_large_grid / _brute   256 large volumes (a 20 m box, the last shape of the table, at random axis-aligned places)
  grid_build_us            the grid path with one query that touches nothing (the passes shared with the ray casts)
  hits_*                   hits in all (both paths give the same lists; checked here)
Device times are the median of --repeats stream-ordered calls of the device variant, timed with HIP events on the world's
stream after a warm-up call; --brute-queries limits the brute-force runs (every query against every body)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch  # first: the library then binds to the HIP runtime torch carries

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from constraint_solver_amd import capi  # noqa: E402


def device_us(w, stream, q, cap, flags, repeats):
    """Median time of the device variant on `stream` (the world's stream), and its answer."""
    with torch.cuda.stream(stream):
        dev_q = torch.from_numpy(q.view(np.uint8).copy()).to("cuda")
        dev_off = torch.zeros(len(q) + 1, dtype=torch.int32, device="cuda")
        dev_hits = torch.empty(max(cap, 1) * 16, dtype=torch.uint8, device="cuda")
        w.overlap_device(dev_q.data_ptr(), len(q), dev_off.data_ptr(), dev_hits.data_ptr(), cap, flags)   # scratch sized, code loaded
        stream.synchronize()
        times = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            w.overlap_device(dev_q.data_ptr(), len(q), dev_off.data_ptr(), dev_hits.data_ptr(), cap, flags)
            b.record(stream)
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        offsets = dev_off.cpu().numpy().view(np.uint32)
        hits = dev_hits.cpu().numpy()[: int(offsets[-1]) * 16].view(capi.OVERLAP_HIT_DTYPE)
    return statistics.median(times), offsets, hits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--frames", type=int, default=120, help="frames the pile settles for")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--small", type=int, default=65536)
    ap.add_argument("--large", type=int, default=256)
    ap.add_argument("--brute-queries", type=int, default=4096, help="queries of the small batch the brute-force path is timed with")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()

    bodies, sid = capi.scene_pile(capi.SCENE_BOXES_DROP, args.seed, args.bodies, 2.0, 4)
    w = capi.World(mode=capi.MODE_CONTACTS)
    w.set_polytopes([capi.polytope(capi.SHAPE_CUBE), capi.polytope(capi.SHAPE_CUBE, 20.0)])
    w.upload(bodies, sid)
    for _ in range(args.frames):
        w.step(1.0 / 60.0, 20)
    state = w.download()
    stream = torch.cuda.Stream()                      # not the null stream: the world's work and the events share one queue
    w.set_stream(stream.cuda_stream)

    rng = np.random.default_rng(args.seed)
    centre = state[:, 31:34] + state[:, 28:31]
    lo, hi = centre.min(axis=0), centre.max(axis=0)
    rot = rng.normal(size=(args.small, 4))
    small = capi.overlap_queries(rng.uniform(lo, hi, (args.small, 3)), rot / np.linalg.norm(rot, axis=1, keepdims=True), 0)
    large = capi.overlap_queries(rng.uniform(lo - 10.0, hi - 10.0, (args.large, 3)), [1.0, 0.0, 0.0, 0.0], 1)
    nothing = capi.overlap_queries([hi + 1000.0], [1.0, 0.0, 0.0, 0.0], 0)

    res = {"bodies": args.bodies, "queries_small": args.small, "queries_large": args.large, "brute_queries": args.brute_queries}
    for name, q in (("small", small), ("large", large)):
        total = len(w.overlap(q)[1])
        t_grid, off_g, hits_g = device_us(w, stream, q, total, 0, args.repeats)
        part = q[: args.brute_queries]
        cap = int(off_g[len(part)])
        t_brute, off_b, hits_b = device_us(w, stream, part, cap, capi.OVERLAP_BRUTE_FORCE, max(1, args.repeats // 3))
        same = off_b.tobytes() == off_g[: len(part) + 1].tobytes() and hits_b.tobytes() == hits_g[:cap].tobytes()
        res.update({"us_%s_grid" % name: t_grid, "us_%s_brute" % name: t_brute, "brute_queries_%s" % name: len(part),
                    "hits_%s" % name: total, "queries_per_s_%s_grid" % name: len(q) / (t_grid * 1e-6), "same_%s" % name: bool(same)})
    res["grid_build_us"] = device_us(w, stream, nothing, 1, 0, args.repeats)[0]
    w.set_stream(0)
    w.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
