#!/usr/bin/env python3
"""Host time of a plan of the sharded world (ns_plan of xpbd_multi_world_plan_stats around xpbd_multi_world_replan) for a
one-device rehearsal: `--shards` shards of a dropped pile of `--bodies` mixed bodies on device 0, XPBD_TRANSPORT_LOCAL.  One frame
is stepped between two re-plans, so every plan finds bodies that moved.  LIGHT plans (the cuts kept) and FULL plans (a world made
with XPBD_MULTI_FULL_PLANS) are timed in worlds of their own.

Without --ab: one JSON line for the library in use (XPBD_HIP_LIB, or the tree's).  With --ab OTHER.so: `--runs` runs of OTHER.so
and of the tree's library in turn, each in a fresh process, and one JSON document with every run, the medians of the runs'
medians and whether the tree's median lies inside the range of the other's runs."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def measure(args):
    from constraint_solver_amd import capi
    kind = capi.SCENE_MIXED_DROP
    bodies, sid = capi.scene_pile(kind, 1, args.bodies, 1.4, 4)
    out = {"library": os.path.basename(os.environ.get("XPBD_HIP_LIB", "libxpbd_hip.so (the tree's)")), "shards": args.shards, "bodies": args.bodies,
           "plans": args.plans, "substeps": args.substeps}
    for mode in ("light", "full"):
        with capi.MultiWorld(args.shards, devices=[0] * args.shards, transport=capi.TRANSPORT_LOCAL, halo_margin=0.75, auto_replan=True,
                             full_plans=mode == "full") as mw:
            mw.set_polytopes(capi.scene_polytopes(kind))
            mw.upload(bodies, sid, 0, args.bodies)
            ms = []
            for i in range(args.warmup + args.plans):
                mw.step(1 / 60, args.substeps)
                mw.synchronize()
                before = mw.plan_stats()
                mw.replan()
                after = mw.plan_stats()
                assert after["plans"] == before["plans"] + 1, (before, after)
                # (a light plan that finds the shards out of balance ends as a full one: not counted among the light plans)
                if i >= args.warmup and after[mode + "_plans"] == before[mode + "_plans"] + 1:
                    ms.append((after["ns_plan"] - before["ns_plan"]) / 1e6)
            out[mode] = {"ms_per_plan": ms, "median_ms": statistics.median(ms), "migrated_at_last_plan": after["migrated"], "halo": mw.halo_stats()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shards", type=int, default=4)
    ap.add_argument("--bodies", type=int, default=65536)
    ap.add_argument("--plans", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--substeps", type=int, default=10)
    ap.add_argument("--ab", metavar="OTHER.so", help="compare with this build of libxpbd_hip.so")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", help="with --ab: write the document here as well")
    args = ap.parse_args()
    if not args.ab:
        print(json.dumps(measure(args)))
        return
    own = [sys.executable, os.path.abspath(__file__)] + [a for k in ("shards", "bodies", "plans", "warmup", "substeps")
                                                        for a in ("--" + k, str(getattr(args, k)))]
    runs = {"other": [], "tree": []}
    for _ in range(args.runs):
        for who in ("other", "tree"):
            env = dict(os.environ)
            env.pop("XPBD_HIP_LIB", None)
            if who == "other":
                env["XPBD_HIP_LIB"] = os.path.abspath(args.ab)
            p = subprocess.run(own, env=env, stdout=subprocess.PIPE, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit("plan_time: a run of the %s library ended with status %d; nothing more is started" % (who, p.returncode))
            runs[who].append(json.loads(p.stdout.strip().splitlines()[-1]))
    doc = {"what": "host ms per plan (ns_plan around xpbd_multi_world_replan), runs of the two libraries in turn", "runs": runs, "summary": {}}
    for mode in ("light", "full"):
        other = [r[mode]["median_ms"] for r in runs["other"]]
        tree = [r[mode]["median_ms"] for r in runs["tree"]]
        doc["summary"][mode] = {"other_median_ms": statistics.median(other), "other_range_ms": [min(other), max(other)],
                                "tree_median_ms": statistics.median(tree), "tree_range_ms": [min(tree), max(tree)],
                                "tree_median_inside_other_range": min(other) <= statistics.median(tree) <= max(other),
                                "tree_median_not_above_other_range": statistics.median(tree) <= max(other)}
    text = json.dumps(doc, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(doc["summary"]))


if __name__ == "__main__":
    main()
