#!/usr/bin/env python3
"""Sensor bodies on bench.py's settled pile (262 144 unit boxes dropped as a pile and pre-rolled to rest; XPBD_MODE_CONTACTS, SAT,
20 substeps): one JSON line, the whole result in --out.  Reads nothing outside the repository (or the --root it is given).

Median [min, max] of --repeats after --warmup, HIP events on the world's stream unless stated:
  (a) ms_frame_empty          one xpbd_world_step of the pile alone, no table: the launches of a world without the feature.  The
                              same figure of the parent commit: run this script with --root <parent checkout> --only-empty,
                              alternating with runs of this tree, and pass the parent's --out files as --parent; the spread of both
                              is reported, no difference is claimed.
  (b) ms_frame_sensors        --slabs fixed boxes of edge --slab-edge on a grid through the pile, flagged as sensors from the start
                              (the pile settles through them), contact report on
      ms_frame_filtered       the same world with the slabs given the filter {0, 0} instead: what the frame costs without the
                              sensor pairs (their narrowphase, the mask kernel, the report's extra pairs)
      (the share of k_sensor_mask_codes itself is a kernel time: take it from a kernel trace of --only-sensors in a run of its own)
  (c) ms_overlaps_device      xpbd_world_sensor_overlaps_device into resident tensors, on the stream
      ms_overlaps_host_pass   xpbd_world_download_pair_contacts (no points) plus a numpy pass that lists every sensor's partners:
                              wall time with the world synchronised, the only route before
--root <tree> imports the package (and bench.py's scene) of another checkout, built there; a tree without the new calls is timed
for ms_frame_empty only."""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--slabs", type=int, default=64)
    ap.add_argument("--slab-edge", type=float, default=8.0)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--preroll", type=int, default=-1, help="frames before anything is timed (default: bench.py's for a pile)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only-empty", action="store_true", help="(a): time ms_frame_empty alone")
    ap.add_argument("--only-sensors", action="store_true", help="(b): run the frames of ms_frame_sensors alone (for a kernel trace)")
    ap.add_argument("--parent", nargs="*", default=[], help="--out files of runs of the parent commit")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch
    import bench
    from constraint_solver_amd import capi

    torch.cuda.set_device(0)
    kind = capi.SCENE_BOXES_DROP
    n = args.bodies
    pile, sid = capi.scene_pile(kind, args.seed, n, 1.8, 4)
    lo, hi = pile[:, 31:34].min(axis=0), pile[:, 31:34].max(axis=0)
    has_calls = hasattr(capi.World, "sensor_overlaps_device") and not args.only_empty
    stream = torch.cuda.current_stream()
    total = args.warmup + args.repeats
    preroll = args.preroll if args.preroll >= 0 else bench.PREROLL_PILE

    def events(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def wall(w, call):
        w.synchronize()
        t0 = time.perf_counter()
        call()
        w.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    def world(bodies, shape_ids, polytopes):
        w = capi.World(mode=capi.MODE_CONTACTS)
        w.set_polytopes(polytopes)
        w.set_contact_pad(0.02)
        w.set_narrowphase(capi.NARROWPHASE_SAT)
        w.upload(bodies, shape_ids)
        w.set_stream(stream.cuda_stream)
        return w

    ms, extra = {}, {}
    if not args.only_sensors:
        with world(pile, sid, capi.scene_polytopes(kind)) as w:
            for _ in range(preroll):
                w.step(bench.FRAME_TIME, args.substeps)
            ms["frame_empty"] = [events(lambda: w.step(bench.FRAME_TIME, args.substeps)) for _ in range(total)]
            extra["finite"] = bool(np.isfinite(w.download()).all())
            w.set_stream(0)
    if has_calls:
        # the slabs: fixed boxes standing on the ground on a grid over the pile's footprint
        m = args.slabs
        side = int(np.ceil(np.sqrt(max(m, 1))))
        slab = np.repeat(pile[:1], m, axis=0)
        slab[:, 0:10] = 0.0
        slab[:, 22:28] = 0.0
        slab[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
        k = np.arange(m)
        slab[:, 31] = lo[0] + (hi[0] - lo[0]) * ((k % side) + 0.5) / side
        slab[:, 32] = lo[1] + (hi[1] - lo[1]) * ((k // side) + 0.5) / side
        slab[:, 33] = 0.0
        bodies = np.concatenate([pile, slab])
        shape_ids = np.concatenate([sid, np.ones(m, dtype=np.uint32)]).astype(np.uint32)
        polytopes = capi.scene_polytopes(kind) + [capi.polytope(capi.SHAPE_CUBE, args.slab_edge)]
        is_sensor = np.zeros(n + m, dtype=np.uint8)
        is_sensor[n:] = 1
        filters = np.zeros(n + m, dtype=capi.COLLISION_FILTER_DTYPE)
        filters["group"] = filters["mask"] = np.where(is_sensor != 0, 0, 0xFFFFFFFF)
        for name in ("frame_sensors",) if args.only_sensors else ("frame_sensors", "frame_filtered"):
            with world(bodies, shape_ids, polytopes) as w:
                w.set_contact_report(True)
                if name == "frame_sensors":
                    w.set_sensors(is_sensor)
                else:
                    w.set_collision_filters(filters)
                for _ in range(preroll):
                    w.step(bench.FRAME_TIME, args.substeps)
                ms[name] = [events(lambda: w.step(bench.FRAME_TIME, args.substeps)) for _ in range(total)]
                if name == "frame_sensors":
                    stats = w.contact_stats()
                    pairs = w.pair_contacts(points=False)[0]
                    sensor_records = int(((is_sensor[pairs["body_a"]] | is_sensor[pairs["body_b"]]) != 0).sum())
                    extra.update(pair_list=stats[0], report_records=len(pairs), sensor_records=sensor_records)
                    if not args.only_sensors:
                        room = 2 * sensor_records + 1
                        dev_sensors = torch.zeros(m, dtype=torch.int32, device="cuda")
                        dev_offsets = torch.zeros(m + 1, dtype=torch.int32, device="cuda")
                        dev_hits = torch.zeros(2 * room, dtype=torch.int32, device="cuda")
                        device = lambda: w.sensor_overlaps_device(dev_sensors.data_ptr(), dev_offsets.data_ptr(), dev_hits.data_ptr(), room)   # noqa: E731
                        ms["overlaps_device"] = [events(device) for _ in range(total)]

                        def host_pass():
                            rec = w.pair_contacts(points=False)[0]
                            a, b = rec["body_a"], rec["body_b"]
                            sa, sb = is_sensor[a] != 0, is_sensor[b] != 0
                            owner = np.concatenate([a[sa], b[sb]])
                            other = np.concatenate([b[sa], a[sb]])
                            order = np.lexsort((other, owner))
                            return owner[order], other[order]

                        ms["overlaps_host_pass"] = [wall(w, host_pass) for _ in range(total)]
                        owner, other = host_pass()
                        offsets = dev_offsets.cpu().numpy().view(np.uint32)
                        got = dev_hits.cpu().numpy().view(np.uint32).reshape(-1, 2)[:offsets[-1], 0]
                        extra["overlaps_agree"] = bool(len(other) == offsets[-1] and np.array_equal(got, other))
                        extra["overlap_hits"] = int(offsets[-1])
                w.set_stream(0)
    own_tree = os.path.abspath(args.root) == os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    result = dict({"tree": "this checkout" if own_tree else "another checkout (--root)", "bodies": n, "slabs": args.slabs, "slab_edge": args.slab_edge,
                   "substeps": args.substeps, "preroll": preroll, "repeats": args.repeats, "warmup": args.warmup}, **extra)
    for name, values in ms.items():
        v = values[args.warmup:]
        if v:
            result["ms_" + name] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
    parents = []
    for path in args.parent:
        with open(path) as f:
            parents.append(json.load(f)["ms_frame_empty"])
    if parents:
        result["parent_commit_ms_frame_empty"] = parents
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(result, what="scripts/sensors_bench.py: sensor slabs through bench.py's settled pile; frames and device calls by HIP events "
                                        "on the world's stream, host passes by wall time with the world synchronised; median [min, max] of %d after %d"
                                        % (args.repeats, args.warmup)), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
