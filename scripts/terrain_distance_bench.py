#!/usr/bin/env python3
"""Batched terrain distance queries on scripts/terrain_bench.py's world -- 262 144 boxes on the rolling 959 x 959 field: one JSON
line, also written to profiles/terrain_distance_bench.json.

  us_points_cell / us_cubes_cell   65 536 point queries / unit-cube queries at random places 0 to 2 m above the ground with max_distance =
                                   one cell of the field: xpbd_world_terrain_distance_device
  us_points_inf / us_cubes_inf     the same with max_distance = +inf
  us_bodies_*                      the yardstick xpbd_world_distance_device with the same queries
  us_overlap_terrain               the yardstick xpbd_world_overlap_device with XPBD_QUERY_TERRAIN and the cubes
  ratio_*                          each terrain time over its yardstick
  samples_floor_*                  per query, the samples of the rings the walk cannot avoid given the FINAL answer (the stop rule
                                   evaluated with the distance the query ended with; the walk, which only knows the best so far, looks at
                                   no fewer): mean and maximum
  same                             one untimed brute-force pass over the first --brute-queries queries of every setting gives the same bits
  runs_us                          every timed call behind the medians; spread_* = (max - min) / median of a setting's calls
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "scripts")]
from constraint_solver_amd import capi  # noqa: E402
from terrain_bench import rolling_field  # noqa: E402

RUNS = {}


def timed(name, stream, call, repeats):
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


def distance_us(name, fn, stream, q, flags, repeats):
    with torch.cuda.stream(stream):
        dev_q = torch.from_numpy(q.view(np.uint8).copy()).to("cuda")
        dev_hits = torch.empty(len(q) * 96, dtype=torch.uint8, device="cuda")
        t = timed(name, stream, lambda: fn(dev_q.data_ptr(), len(q), dev_hits.data_ptr(), flags), repeats)
        return t, dev_hits.cpu().numpy().view(capi.DISTANCE_HIT_DTYPE)


def samples_floor(field, q, hits, radius):
    """Per query the samples in the rings 0 .. r, r the last ring the stop rule admits with the query's final distance."""
    heights, origin, cell = field
    ny, nx = heights.shape
    reach = radius + np.minimum(np.where(hits["body"] == capi.NO_HIT, np.inf, hits["distance"]), q["max_distance"])
    ci = np.clip(np.floor((q["position"][:, 0] - origin[0]) / cell[0]), 0, nx - 1)
    cj = np.clip(np.floor((q["position"][:, 1] - origin[1]) / cell[1]), 0, ny - 1)
    fx, fy = q["position"][:, 0] - (origin[0] + ci * cell[0]), q["position"][:, 1] - (origin[1] + cj * cell[1])
    # ring r is admitted while the nearest of its four inner borders is within reach: r - 1 whole cells plus the nearer remainder
    near = np.minimum(np.minimum(fx, cell[0] - fx), np.minimum(fy, cell[1] - fy))
    r = np.where(np.isfinite(reach), np.floor(np.maximum(reach - near, 0.0) / min(cell)) + 1, max(nx, ny))
    r = np.minimum(r, max(nx, ny))
    count = (np.minimum(ci + r, nx - 1) - np.maximum(ci - r, 0) + 1) * (np.minimum(cj + r, ny - 1) - np.maximum(cj - r, 0) + 1)
    return {"mean": float(count.mean()), "max": int(count.max())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--preroll", type=int, default=60, help="frames the boxes settle for")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--queries", type=int, default=65536)
    ap.add_argument("--brute-queries", type=int, default=1024)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "terrain_distance_bench.json"))
    args = ap.parse_args()

    kind = capi.SCENE_BOXES_DROP
    bodies, sid = capi.scene_pile(kind, args.seed, args.bodies, 1.8, 4)
    field = rolling_field(bodies, 0.3, 4.0)
    heights, origin, cell = field
    w = capi.World(mode=capi.MODE_CONTACTS)
    w.set_polytopes(capi.scene_polytopes(kind))
    w.set_narrowphase(capi.NARROWPHASE_SAT)
    w.set_terrain(*field)
    start = bodies.copy()
    start[:, 33] += w.sample_terrain(bodies[:, 31:33] + bodies[:, 28:30], normals=False) + 0.3
    w.upload(start, sid)
    for _ in range(args.preroll):
        w.step(1.0 / 60.0, 20)
    state = w.download()
    stream = torch.cuda.Stream()                      # not the null stream: the world's work and the events share one queue
    w.set_stream(stream.cuda_stream)

    rng = np.random.default_rng(args.seed)
    n = args.queries
    centre = state[:, 31:33] + state[:, 28:30]
    xy = rng.uniform(centre.min(axis=0), centre.max(axis=0), (n, 2))
    pos = np.column_stack([xy, w.sample_terrain(xy, normals=False) + rng.uniform(0.0, 2.0, n)])
    rot = rng.normal(size=(n, 4))
    rot /= np.linalg.norm(rot, axis=1, keepdims=True)
    res = {"bodies": args.bodies, "queries": n, "field_samples": [heights.shape[1], heights.shape[0]], "cell": cell[0],
           "brute_queries": args.brute_queries, "repeats": args.repeats}
    same = True
    cube_radius = float(np.sqrt(0.75))
    for reach_name, reach in (("cell", cell[0]), ("inf", np.inf)):
        for shape_name, q, radius in (("points", capi.distances(pos, max_distance=reach), 0.0), ("cubes", capi.distances(pos, rot, 0, max_distance=reach), cube_radius)):
            key = "%s_%s" % (shape_name, reach_name)
            t, hits = distance_us("terrain_" + key, w.terrain_distance_device, stream, q, 0, args.repeats)
            t_bodies, _ = distance_us("bodies_" + key, w.distance_device, stream, q, 0, args.repeats)
            part = q[: args.brute_queries]
            same = same and w.terrain_distance(part, capi.DISTANCE_BRUTE_FORCE).tobytes() == hits[: len(part)].tobytes()
            found = hits["body"] == capi.HIT_TERRAIN
            res.update({"us_" + key: t, "us_bodies_" + key: t_bodies, "ratio_%s_to_bodies" % key: t / t_bodies, "queries_per_s_" + key: n / (t * 1e-6),
                        "answers_" + key: int(found.sum()), "overlaps_" + key: int((found & (hits["feature"] == capi.DISTANCE_OVERLAP)).sum()),
                        "samples_floor_" + key: samples_floor(field, q, hits, radius),
                        "spread_" + key: (max(RUNS["terrain_" + key]) - min(RUNS["terrain_" + key])) / t})
    volumes = capi.overlap_queries(pos, rot, 0)
    total = len(w.overlap(volumes, capi.QUERY_TERRAIN)[1])
    with torch.cuda.stream(stream):
        dev_q = torch.from_numpy(volumes.view(np.uint8).copy()).to("cuda")
        dev_off = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        dev_hits = torch.empty(max(total, 1) * 16, dtype=torch.uint8, device="cuda")
        t_overlap = timed("overlap_terrain", stream, lambda: w.overlap_device(dev_q.data_ptr(), n, dev_off.data_ptr(), dev_hits.data_ptr(), total,
                                                                               capi.QUERY_TERRAIN), args.repeats)
    res.update({"us_overlap_terrain": t_overlap, "overlap_hits": total, "same": bool(same), "runs_us": RUNS})
    for key in ("points_cell", "cubes_cell", "points_inf", "cubes_inf"):
        res["ratio_%s_to_overlap" % key] = res["us_" + key] / t_overlap
    w.set_stream(0)
    w.close()
    line = json.dumps(res)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
