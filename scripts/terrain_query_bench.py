#!/usr/bin/env python3
"""What the terrain costs in the scene queries: scripts/terrain_bench.py's world (262 144 unit boxes in 4 layers settled on the
rolling 959 x 959 field) asked 1 M random rays, 65 536 sweeps and 65 536 overlap queries, each family without and with
XPBD_QUERY_TERRAIN, through the device variants (torch tensors; torch is imported first so that the library binds to the HIP
runtime torch carries, as in bench.py).  A call is timed from its enqueue to the world's synchronize; every figure is the median
of `--runs` calls with their min and max.

A library without the flag (an older build loaded through XPBD_HIP_LIB, for the "no change without the flag" comparison: run the
script once per library, same process order) reports the unflagged calls only.  One JSON object; --out also writes it.

--merge OUT FILE...: no measurement; the objects of several processes (files written with --out, in the order the processes ran)
become one document: every process as it was, and per family a summary -- the medians over all timed calls of this tree's
library and of the other one, their difference, the other library's own min-to-max spread, the flagged calls of this tree.
profiles/terrain_query_bench.json is such a document."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from constraint_solver_amd import capi  # noqa: E402
from terrain_bench import rolling_field  # noqa: E402

T, HIT_TERRAIN = capi.QUERY_TERRAIN, capi.HIT_TERRAIN
FAMILIES = ("rays", "sweeps", "overlaps")


def unit_quaternions(rng, n):
    q = rng.normal(size=(n, 4))
    return q / np.linalg.norm(q, axis=1, keepdims=True)


def rounded(x):
    if isinstance(x, float):
        return round(x, 4)
    if isinstance(x, list):
        return [rounded(v) for v in x]
    if isinstance(x, dict):
        return {k: rounded(v) for k, v in x.items()}
    return x


def merge(out, files):
    runs, names, count = [], [], {"tree": 0, "parent": 0}
    for path in files:
        with open(path) as f:
            runs.append(json.load(f))
        kind = "tree" if runs[-1]["library"] == "this tree's" else "parent"
        count[kind] += 1
        names.append("%s_%d" % (kind, count[kind]))
    doc = {"what": "scripts/terrain_query_bench.py, one process per entry of `processes` in the order they ran (tree: this tree's library; parent: "
                   "another build through XPBD_HIP_LIB, which has no flag), merged by --merge; ms per call, device variants",
           "field": runs[0]["field"], "bodies": runs[0]["bodies"],
           "processes": {name: {fam: rounded({k: v for k, v in r[fam].items() if k != "count"}) for fam in FAMILIES} for name, r in zip(names, runs)},
           "summary": {}}
    for fam in FAMILIES:
        calls = {kind: [t for name, r in zip(names, runs) if name.startswith(kind) for t in r[fam]["plain"]["ms_runs"]] for kind in count}
        flagged = [t for name, r in zip(names, runs) if name.startswith("tree") for t in r[fam]["terrain"]["ms_runs"]]
        n = runs[0][fam]["count"]
        entry = {"count": n, "plain_ms_median_this_tree": statistics.median(calls["tree"]), "plain_per_s": n / (1e-3 * statistics.median(calls["tree"])),
                 "terrain_ms_median": statistics.median(flagged), "terrain_ms_min_max": [min(flagged), max(flagged)],
                 "terrain_per_s": n / (1e-3 * statistics.median(flagged))}
        if calls["parent"]:
            pm = statistics.median(calls["parent"])
            entry.update({"plain_ms_median_parent": pm, "plain_difference_percent": 100.0 * (entry["plain_ms_median_this_tree"] - pm) / pm,
                          "parent_run_to_run_spread_percent": 100.0 * (max(calls["parent"]) - min(calls["parent"])) / pm})
        doc["summary"][fam] = rounded(entry)
    with open(out, "w") as f:
        f.write(json.dumps(doc, indent=1) + "\n")
    print(json.dumps(doc["summary"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--merge", nargs="+", default=None, metavar="FILE", help="OUT FILE...: merge the objects of several processes, measure nothing")
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--amplitude", type=float, default=0.3)
    ap.add_argument("--wavelength", type=float, default=4.0)
    ap.add_argument("--preroll", type=int, default=183)
    ap.add_argument("--rays", type=int, default=1 << 20)
    ap.add_argument("--volumes", type=int, default=65536)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.merge:
        return merge(args.merge[0], args.merge[1:])
    torch.cuda.set_device(0)
    kind, n, dt = capi.SCENE_BOXES_DROP, args.bodies, 1.0 / 60.0
    bodies, sid = capi.scene_pile(kind, args.seed, n, 1.8, 4)
    heights, origin, cell = rolling_field(bodies, args.amplitude, args.wavelength)
    rng = np.random.default_rng(args.seed)
    lo = np.array(origin)
    hi = lo + [(heights.shape[1] - 1) * cell[0], (heights.shape[0] - 1) * cell[1]]
    result = {"library": os.environ.get("XPBD_HIP_LIB", "this tree's"), "bodies": n, "runs": args.runs,
              "field": {"samples": [heights.shape[1], heights.shape[0]], "cell": cell[0],
                        "plane_table_MiB": (heights.shape[0] - 1) * (heights.shape[1] - 1) * 64 / 2.0**20}}
    w = capi.World(mode=capi.MODE_CONTACTS)
    try:
        w.set_polytopes(capi.scene_polytopes(kind))
        w.set_narrowphase(capi.NARROWPHASE_SAT)
        w.set_terrain(heights, origin, cell)
        start = bodies.copy()
        start[:, 33] += w.sample_terrain(bodies[:, 31:33] + bodies[:, 28:30], normals=False) + abs(args.amplitude)
        w.upload(start, sid)
        for _ in range(args.preroll):
            w.step(dt, args.substeps)
        w.synchronize()
        top = float(w.download()[:, 33].max()) + 2.0
        # rays: origins over the field and a margin around it, from the ground to above the pile, directions anywhere in the lower
        # half-space and some in the upper, every third one bounded
        k = args.rays
        o = np.stack([rng.uniform(lo[0] - 5.0, hi[0] + 5.0, k), rng.uniform(lo[1] - 5.0, hi[1] + 5.0, k), rng.uniform(0.5, top + 6.0, k)], axis=1)
        d = rng.normal(size=(k, 3))
        d[:, 2] -= 0.7
        rays = capi.rays(o, d, np.where(np.arange(k) % 3 == 0, 20.0, np.inf))
        # volumes: unit boxes at random rotations; sweeps fall or slide from above the pile and beside it, overlap volumes sit
        # around the ground and in the pile
        v = args.volumes
        pos = np.stack([rng.uniform(lo[0], hi[0], v), rng.uniform(lo[1], hi[1], v), rng.uniform(0.0, top + 2.0, v)], axis=1)
        sd = rng.normal(size=(v, 3)) * [1.0, 1.0, 0.3]
        sd[:, 2] -= 0.6
        sweeps = capi.sweeps(pos, unit_quaternions(rng, v), sd, 0, max_distance=np.where(np.arange(v) % 3 == 0, 10.0, np.inf))
        pos = np.stack([rng.uniform(lo[0], hi[0], v), rng.uniform(lo[1], hi[1], v), rng.uniform(-0.5, 0.6 * top, v)], axis=1)
        queries = capi.overlap_queries(pos, unit_quaternions(rng, v), 0)
        dev = {name: torch.from_numpy(batch.view(np.uint8).copy()).to("cuda") for name, batch in (("rays", rays), ("sweeps", sweeps), ("overlaps", queries))}
        ray_hits = torch.zeros(k * 64, dtype=torch.uint8, device="cuda")
        sweep_hits = torch.zeros(v * 72, dtype=torch.uint8, device="cuda")
        cap = 64 * v
        offsets = torch.zeros(v + 1, dtype=torch.int32, device="cuda")
        overlap_hits = torch.zeros(cap * 16, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        calls = {"rays": (k, lambda f: w.raycast_device(dev["rays"].data_ptr(), k, ray_hits.data_ptr(), f)),
                 "sweeps": (v, lambda f: w.sweep_device(dev["sweeps"].data_ptr(), v, sweep_hits.data_ptr(), f)),
                 "overlaps": (v, lambda f: w.overlap_device(dev["overlaps"].data_ptr(), v, offsets.data_ptr(), overlap_hits.data_ptr(), cap, f))}

        def census(name):
            """How the answers of the last call divide between the terrain, the bodies and nothing."""
            if name == "rays":
                body = np.frombuffer(ray_hits.cpu().numpy().tobytes(), dtype=capi.RAY_HIT_DTYPE)["body"]
            elif name == "sweeps":
                body = np.frombuffer(sweep_hits.cpu().numpy().tobytes(), dtype=capi.SWEEP_HIT_DTYPE)["body"]
            else:
                total = int(offsets.cpu().numpy()[-1])
                body = np.frombuffer(overlap_hits.cpu().numpy().tobytes(), dtype=capi.OVERLAP_HIT_DTYPE)["body"][:min(total, cap)]
                return {"entries": total, "terrain": int((body == HIT_TERRAIN).sum())}
            return {"terrain": int((body == HIT_TERRAIN).sum()), "miss": int((body == capi.NO_HIT).sum()),
                    "bodies": int(((body != HIT_TERRAIN) & (body != capi.NO_HIT)).sum())}

        for name, (count, call) in calls.items():
            result[name] = {"count": count}
            for label, flags in (("plain", 0), ("terrain", T)):
                try:
                    call(flags)                                 # warm-up: the scratch grows here
                except capi.XpbdError:
                    if flags == 0:
                        raise
                    continue                                    # a library without the flag
                w.synchronize()
                times = []
                for _ in range(args.runs):
                    t0 = time.perf_counter()
                    call(flags)
                    w.synchronize()
                    times.append(time.perf_counter() - t0)
                median = statistics.median(times)
                result[name][label] = {"ms_median": 1e3 * median, "ms_min": 1e3 * min(times), "ms_max": 1e3 * max(times),
                                       "ms_runs": [1e3 * t for t in times], "per_s": count / median, "answers": census(name)}
    finally:
        w.close()
    text = json.dumps(result)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
