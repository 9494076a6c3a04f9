#!/usr/bin/env python3
"""Mass edits on bench.py's scenes: --scene pile, the settled pile of 262 144 unit boxes (SAT, 20 substeps), or --scene joints, the
262 144 boxes + 65 408 joints scene with a drive on every hinge and a friction coefficient per body.  One JSON line, the whole
result in --out.

Median [min, max] of --repeats after --warmup; device calls by HIP events on the world's stream, host calls by wall time with the
world synchronised (they wait):
  (ii) ms_frame_shared       one xpbd_world_step before any edit: the contact pipeline reads the per-shape mass table
       ms_frame_per_body     the same after ONE body was given its own row again: the world has left the shared table for the
                             per-body records (the price of an edit, paid from then on until the next upload)
  (i)  ms_set_device_all / _1pct, ms_set_host_all / _1pct   xpbd_world_set_mass_properties(_device), every row / every 100th
       ms_get_host_all       xpbd_world_get_mass_properties of every body
       ms_reupload           the only route before: xpbd_world_download_bodies, the 13 columns written on the host,
                             xpbd_world_upload_bodies, joints / drives / materials set again
Every row written is the row the body already has, so the scene stays the one that was pre-rolled.  (iii), a world that never
calls the new entry points against the parent commit, is bench.py itself run on both trees.
--root <tree> imports the package (and bench.py's scenes) of another checkout, built there; a tree without the new calls is timed
for ms_frame_shared and ms_reupload only."""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--scene", choices=["pile", "joints"], default="pile")
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--joints", type=int, default=65408)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--preroll", type=int, default=-1, help="frames before anything is timed (default: bench.py's for the scene)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
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
    joints = drives = friction = None
    if args.scene == "pile":
        state, sid = capi.scene_pile(kind, args.seed, n, 1.8, 4)
        preroll = bench.PREROLL_PILE
    else:
        grid_w = bench.scene_grid_width(capi, kind, n, n)
        state, sid = capi.scene_generate(kind, args.seed, n, grid_w=grid_w)
        joints = bench.chain_joints(capi, np, args.joints, n, 2.0, grid_w, state=state)
        hinges = np.nonzero(joints["kind"] == capi.JOINT_HINGE)[0]
        drives = np.zeros(len(hinges), dtype=capi.JOINT_DRIVE_DTYPE)
        drives["joint"], drives["kind"], drives["target"], drives["max_force"] = hinges, capi.DRIVE_ANGULAR_VELOCITY, 1.0, np.inf
        for side in "ab":                                      # a unit reference perpendicular to each (unit) axis
            axis = joints["axis_" + side][hinges]
            ref = np.cross(axis, np.where(np.abs(axis[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]]))
            drives["ref_" + side] = ref / np.linalg.norm(ref, axis=1, keepdims=True)
        friction = np.full(n, 0.5)
        preroll = bench.PREROLL["boxes-drop"]
    if args.preroll >= 0:
        preroll = args.preroll
    has_calls = hasattr(capi.World, "set_mass_properties_device")
    stream = torch.cuda.current_stream()
    total = args.warmup + args.repeats
    mass_columns = list(range(0, 10)) + [28, 29, 30]

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

    def settings(w):
        if joints is not None:
            w.set_joints(joints)
            w.set_joint_drives(drives)
            w.set_materials(friction, 0.5)

    ms = {}
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(kind))
        w.set_contact_pad(0.02)
        w.set_narrowphase(capi.NARROWPHASE_SAT)
        w.upload(state, sid)
        settings(w)
        w.set_stream(stream.cuda_stream)
        for _ in range(preroll):
            w.step(bench.FRAME_TIME, args.substeps)
        frame = lambda: w.step(bench.FRAME_TIME, args.substeps)   # noqa: E731
        ms["frame_shared"] = [events(frame) for _ in range(total)]
        unchanged = None
        if has_calls:
            w.set_mass_properties([n // 2], w.get_mass_properties([n // 2]))       # one body, its own row: the shared table is left
            ms["frame_per_body"] = [events(frame) for _ in range(total)]
            before = w.download()
            rows = w.get_mass_properties()
            every = np.arange(n, dtype=np.uint32)
            for tag, idx in (("all", every), ("1pct", np.ascontiguousarray(every[::100]))):
                dev_idx = torch.from_numpy(idx.view(np.int32).copy()).cuda()
                dev_rows = torch.from_numpy(np.ascontiguousarray(rows[idx])).cuda()
                host_rows = np.ascontiguousarray(rows[idx])
                ms["set_device_" + tag] = [events(lambda: w.set_mass_properties_device(dev_idx.data_ptr(), len(idx), dev_rows.data_ptr(), capi.MASS_INVERSE))
                                           for _ in range(total)]
                ms["set_host_" + tag] = [wall(w, lambda: w.set_mass_properties(idx, host_rows)) for _ in range(total)]
            ms["get_host_all"] = [wall(w, w.get_mass_properties) for _ in range(total)]
            unchanged = before.tobytes() == w.download().tobytes()

        def reupload():
            b = w.download()
            b[:, mass_columns] = b[:, mass_columns]               # the edit, on the host
            w.upload(b, sid)
            settings(w)

        ms["reupload"] = [wall(w, reupload) for _ in range(total)]
        finite = bool(np.isfinite(w.download()).all())
        w.set_stream(0)
    own_tree = os.path.abspath(args.root) == os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    result = {"tree": "this checkout" if own_tree else "another checkout (--root)", "scene": args.scene, "bodies": n,
              "joints": 0 if joints is None else len(joints), "drives": 0 if drives is None else len(drives), "substeps": args.substeps,
              "repeats": args.repeats, "warmup": args.warmup, "finite": finite, "rows_written_left_the_world_unchanged": unchanged}
    base = statistics.median(ms["frame_shared"][args.warmup:])
    for name, values in ms.items():
        v = values[args.warmup:]
        if v:
            result["ms_" + name] = {"median": statistics.median(v), "min": min(v), "max": max(v), "of_frame_shared": statistics.median(v) / base}
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(result, what="scripts/mass_edit_bench.py: mass edits on bench.py's scenes; frames and device calls by HIP events on the "
                                        "world's stream, host calls by wall time with the world synchronised; median [min, max] of %d after %d"
                                        % (args.repeats, args.warmup)), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
