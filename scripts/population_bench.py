#!/usr/bin/env python3
"""Population changes on bench.py's joints scene (262 144 unit boxes, 65 408 joints, XPBD_MODE_CONTACTS; plus a collision-filter,
a friction and a restitution table, so that every gather runs): one JSON line.

  new_ms        (a) a random 1 % of the bodies removed and as many appended through xpbd_world_remove_bodies / _add_bodies
  reupload_ms   (b) the only route there was before: xpbd_world_download_bodies, the edit in numpy, xpbd_world_upload_bodies,
                joints re-indexed on the host, and every setting set again
Both routes run in the same process on the same world, alternating, --runs times each; every call waits, so the figures are wall
clock around the calls (time.perf_counter).  Medians and ranges; `gain_holds` is the project's rule for a gain: the slowest
run of (a) beats the fastest run of (b).  Recorded, not gated.

With --trace-csv the kernel trace of a run under `rocprofv3 --kernel-trace` (its *_kernel_trace.csv) adds the body gather's
own time and achieved bytes/s: per surviving body 38 doubles and a shape id read and written, 4 bytes of the source map read."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np
import torch  # first: the library then binds to the HIP runtime torch carries  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the joints scene is bench.py's)
from constraint_solver_amd import capi  # noqa: E402

NO_HIT = capi.NO_HIT


def reindex(joints, keep):
    """Joints after the bodies with keep[i] == False left: numpy, what a host had to do by hand."""
    old_to_new = np.where(keep, np.cumsum(keep) - 1, NO_HIT).astype(np.uint32)
    alive = keep[joints["body_a"]] & keep[joints["body_b"]]
    out = joints[alive].copy()
    out["body_a"], out["body_b"] = old_to_new[out["body_a"]], old_to_new[out["body_b"]]
    return out


def gather_from_trace(path, n_keep):
    rows = [r for r in csv.DictReader(open(path)) if "k_population_gather_bodies" in r["Kernel_Name"]]
    if not rows:
        return {}
    us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows]
    moved = n_keep * (2 * (38 * 8 + 4) + 4)
    return {"gather_bodies_dispatches": len(us), "gather_bodies_us_median": statistics.median(us), "gather_bodies_us_min": min(us),
            "gather_bodies_us_max": max(us), "gather_bodies_bytes": moved, "gather_bodies_gbytes_per_s": moved / (statistics.median(us) * 1e3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--joints", type=int, default=65536)
    ap.add_argument("--fraction", type=float, default=0.01)
    ap.add_argument("--preroll", type=int, default=5, help="frames the scene runs before anything is timed")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only-new", action="store_true", help="route (a) alone (for a kernel trace)")
    ap.add_argument("--trace-csv", default="", help="a rocprofv3 *_kernel_trace.csv of an --only-new run: adds the gather kernel's figures")
    ap.add_argument("--out", default="", help="also write the JSON to this file")
    args = ap.parse_args()
    n, kind, pitch = args.bodies, capi.SCENE_BOXES_DROP, 2.0
    grid_w = bench.scene_grid_width(capi, kind, n, n)
    state, sid = capi.scene_generate(kind, args.seed, n, grid_w=grid_w)
    joints = bench.chain_joints(capi, np, args.joints, n, pitch, grid_w, state=state)
    rng = np.random.default_rng(args.seed)
    filters = np.zeros(n, dtype=capi.COLLISION_FILTER_DTYPE)
    filters["group"], filters["mask"] = 1 << rng.integers(0, 4, n), 0xF
    mu, e = rng.uniform(0.2, 0.9, n), rng.uniform(0.0, 0.5, n)
    k = max(int(n * args.fraction), 1)
    new_ms, old_ms = [], []
    n_joints0 = len(joints)
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(kind))
        w.upload(state, sid)

        def set_all():
            w.set_joints(joints)
            w.set_collision_filters(filters, capi.FILTER_JOINTED)
            w.set_materials(mu, 0.6)
            w.set_restitution(e, 0.3, 0.1)

        set_all()
        for _ in range(args.preroll):
            w.step(1.0 / 60.0, 20)
        w.synchronize()
        default_filter = np.zeros(k, dtype=capi.COLLISION_FILTER_DTYPE)
        default_filter["group"] = default_filter["mask"] = 0xFFFFFFFF
        for r in range(args.runs):
            for route in ("new",) if args.only_new else ("new", "reupload"):
                removed = rng.choice(n, k, replace=False).astype(np.uint32)
                fresh, fresh_sid = capi.scene_generate(kind, args.seed + 1 + r, k, grid_w=grid_w)
                fresh[:, 33] += 40.0
                keep = np.ones(n, dtype=bool)
                keep[removed] = False
                if route == "new":
                    t0 = time.perf_counter()
                    w.remove_bodies(removed)
                    w.add_bodies(fresh, fresh_sid)
                    new_ms.append((time.perf_counter() - t0) * 1e3)
                    joints = reindex(joints, keep)                       # (the host copies follow, outside the timed region)
                    filters = np.concatenate([filters[keep], default_filter])
                    mu, e = np.concatenate([mu[keep], np.full(k, np.inf)]), np.concatenate([e[keep], np.zeros(k)])
                    sid = np.concatenate([sid[keep], fresh_sid])
                    assert w.n_joints == len(joints)
                else:
                    t0 = time.perf_counter()
                    now = w.download()
                    now = np.concatenate([now[keep], fresh])
                    sid = np.concatenate([sid[keep], fresh_sid])
                    joints = reindex(joints, keep)
                    filters = np.concatenate([filters[keep], default_filter])
                    mu, e = np.concatenate([mu[keep], np.full(k, np.inf)]), np.concatenate([e[keep], np.zeros(k)])
                    w.upload(now, sid)
                    set_all()
                    old_ms.append((time.perf_counter() - t0) * 1e3)
        w.step(1.0 / 60.0, 20)                                           # the world is still a world
        finite = bool(np.isfinite(w.download()).all())
    result = {"bodies": n, "joints_at_start": n_joints0, "joints_at_end": int(len(joints)), "changed_per_run": k, "runs": args.runs,
              "new_ms": new_ms, "new_ms_median": statistics.median(new_ms), "new_ms_range": [min(new_ms), max(new_ms)], "finite": finite}
    if old_ms:
        result.update({"reupload_ms": old_ms, "reupload_ms_median": statistics.median(old_ms), "reupload_ms_range": [min(old_ms), max(old_ms)],
                       "speedup_of_medians": statistics.median(old_ms) / statistics.median(new_ms), "gain_holds": max(new_ms) < min(old_ms)})
    if args.trace_csv:
        result.update(gather_from_trace(args.trace_csv, n - k))
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
