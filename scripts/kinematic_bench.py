#!/usr/bin/env python3
"""Kinematic bodies on bench.py's settled pile (262 144 unit boxes dropped as a pile and pre-rolled to rest; SAT, 20 substeps)
with ONE fixed unit box added beside the pile as the kinematic body: one JSON line, the whole result in --out.

The scene polytopes hold no slab wide enough to carry the pile, so the kinematic body stands beside it and sweeps into its edge;
what (a) measures -- the unfused schedule and the overwrite kernel against the fused schedule -- does not depend on where it is.

Median [min, max] of --repeats after --warmup, HIP events on the world's stream unless stated:
  (a) ms_frame_empty        one xpbd_world_step with an empty table: the fused schedule, the launches of a world without the feature
      ms_frame_held         the table holds the box at its pose: the unfused schedule plus k_kinematic_velocities, nothing MOVING
      ms_frame_moving       the box travels 1 cm per frame into the pile (a new POSE target before every frame, on the stream)
  (b) ms_retarget_device    xpbd_world_set_kinematic_targets_device for --kinematic fixed boxes on a far grid, all entries
      ms_retarget_host      xpbd_world_set_kinematic_targets for the same entries: wall time with the world synchronised (it waits)
      ms_set_dynamics       xpbd_world_set_dynamics for the same bodies, wall time: the only route before
  (c) ms_frame_empty of this tree against the same figure of the parent commit: run this script with --root <parent checkout>
      --only-empty, alternating with runs of this tree, and pass the parent's --out files as --parent; the spread of both is
      reported, no difference is claimed.
--root <tree> imports the package (and bench.py's scene) of another checkout, built there; a tree without the new calls is timed
for ms_frame_empty and ms_set_dynamics only."""
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
    ap.add_argument("--kinematic", type=int, default=4096)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--preroll", type=int, default=-1, help="frames before anything is timed (default: bench.py's for a pile)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--only-empty", action="store_true", help="(c): time ms_frame_empty alone")
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
    # the kinematic box: fixed, on the ground, half a metre outside the pile's edge as dropped, half way along it
    box = pile[:1].copy()
    box[0, 0:10] = 0.0
    box[0, 22:28] = 0.0
    box[0, 34:38] = [1.0, 0.0, 0.0, 0.0]
    box[0, 31:34] = [lo[0] - 1.5, 0.5 * (lo[1] + hi[1]), 0.0]
    # (b): a grid of fixed boxes far from the pile, 3 m apart, 5 m up
    m = args.kinematic
    side = int(np.ceil(np.sqrt(max(m, 1))))
    far = np.repeat(box, m, axis=0)
    far[:, 31] = hi[0] + 100.0 + 3.0 * (np.arange(m) % side)
    far[:, 32] = lo[1] + 3.0 * (np.arange(m) // side)
    far[:, 33] = 5.0
    state = np.concatenate([pile, box, far])
    sid = np.concatenate([sid, np.zeros(1 + m, dtype=np.uint32)])
    slab = n
    has_calls = hasattr(capi.World, "set_kinematic_targets_device") and not args.only_empty
    stream = torch.cuda.current_stream()
    total = args.warmup + args.repeats

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

    ms = {}
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(kind))
        w.set_contact_pad(0.02)
        w.set_narrowphase(capi.NARROWPHASE_SAT)
        w.upload(state, sid)
        w.set_stream(stream.cuda_stream)
        for _ in range(args.preroll if args.preroll >= 0 else bench.PREROLL_PILE):
            w.step(bench.FRAME_TIME, args.substeps)
        frame = lambda: w.step(bench.FRAME_TIME, args.substeps)   # noqa: E731
        ms["frame_empty"] = [events(frame) for _ in range(total)]
        far_idx = np.arange(slab + 1, slab + 1 + m, dtype=np.uint32)
        far_rows = w.get_dynamics(far_idx)
        ms["set_dynamics"] = [wall(w, lambda: w.set_dynamics(far_idx, far_rows)) for _ in range(total)] if m else []
        if has_calls:
            at = w.get_dynamics([slab])[0]
            held = capi.kinematics([slab], capi.KINEMATIC_POSE, [at[0:3]], [at[3:7]])
            w.set_kinematics(held)
            ms["frame_held"] = [events(frame) for _ in range(total)]
            row = torch.from_numpy(np.concatenate([at[0:3], at[3:7]])).cuda()

            def moving_frame():
                row[0] += 0.01                                      # on the stream: no host copy inside the loop
                w.set_kinematic_targets_device(None, row.data_ptr(), 1)
                w.step(bench.FRAME_TIME, args.substeps)

            ms["frame_moving"] = [events(moving_frame) for _ in range(total)]
            if m:
                rows = far_rows[:, 0:7].copy()
                w.set_kinematics(capi.kinematics(far_idx, capi.KINEMATIC_POSE, rows[:, 0:3], rows[:, 3:7]))
                dev_rows = torch.from_numpy(rows).cuda()
                ms["retarget_device"] = [events(lambda: w.set_kinematic_targets_device(None, dev_rows.data_ptr(), m)) for _ in range(total)]
                ms["retarget_host"] = [wall(w, lambda: w.set_kinematic_targets(None, rows)) for _ in range(total)]
            w.set_kinematics(None)
            ms["frame_empty_again"] = [events(frame) for _ in range(total)]   # (c) within one run: the table cleared
        finite = bool(np.isfinite(w.download()).all())
        w.set_stream(0)
    own_tree = os.path.abspath(args.root) == os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    result = {"tree": "this checkout" if own_tree else "another checkout (--root)", "bodies": n, "kinematic": m, "substeps": args.substeps,
              "repeats": args.repeats, "warmup": args.warmup, "finite": finite}
    base = statistics.median(ms["frame_empty"][args.warmup:])
    for name, values in ms.items():
        v = values[args.warmup:]
        if v:
            result["ms_" + name] = {"median": statistics.median(v), "min": min(v), "max": max(v), "of_frame_empty": statistics.median(v) / base}
    parents = []
    for path in args.parent:
        with open(path) as f:
            parents.append(json.load(f)["ms_frame_empty"])
    if parents:
        result["parent_commit_ms_frame_empty"] = parents
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(result, what="scripts/kinematic_bench.py: kinematic bodies beside bench.py's settled pile; frames and device calls by HIP "
                                        "events on the world's stream, host calls by wall time with the world synchronised; median [min, max] of "
                                        "%d after %d" % (args.repeats, args.warmup)), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
