#!/usr/bin/env python3
"""Joint states and drive targets on bench.py's joints scene (262 144 unit boxes, 65 408 joints in chains of five, an
XPBD_DRIVE_ANGULAR_VELOCITY drive on each of the 16 352 hinges; SAT, 20 substeps): one JSON line, the whole result in --out.

After bench.py's pre-roll, median [min, max] of --repeats after --warmup, each also as a fraction of one frame:
  ms_frame                 one xpbd_world_step, HIP events on the world's stream
  ms_states_device         xpbd_world_joint_states_device, all joints, HIP events
  ms_states_host           xpbd_world_joint_states, all joints: wall time with the world synchronised (it waits)
  ms_download_bodies       xpbd_world_download_bodies alone, wall time: what a host needed before (the atan2s came on top)
  ms_targets_device_all / _1pct   xpbd_world_set_drive_targets_device, all drives / every hundredth, HIP events
  ms_targets_host_all / _1pct     xpbd_world_set_drive_targets, wall time
  ms_set_joint_drives      xpbd_world_set_joint_drives of the whole table, wall time: the only route before
--root <tree> imports the package (and bench.py's scene) of another checkout, built there; a tree without the new calls is
timed for ms_frame, ms_download_bodies and ms_set_joint_drives only.  --parent <json>: the --out of such a run of the parent
commit, stored beside this tree's figures, so that the whole-table setter is quoted as the parent ran it."""
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
    ap.add_argument("--joints", type=int, default=65536)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--preroll", type=int, default=-1, help="frames before anything is timed (default: bench.py's for the scene)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--parent", default="")
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
    n_joints, n_drives = len(joints), len(drives)
    has_calls = hasattr(capi.World, "set_drive_targets_device")
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
        w.set_joints(joints)
        w.set_joint_drives(drives)
        w.set_stream(stream.cuda_stream)
        for _ in range(args.preroll if args.preroll >= 0 else bench.PREROLL["boxes-drop"]):
            w.step(bench.FRAME_TIME, args.substeps)
        ms["frame"] = [events(lambda: w.step(bench.FRAME_TIME, args.substeps)) for _ in range(total)]
        ms["download_bodies"] = [wall(w, w.download) for _ in range(total)]
        ms["set_joint_drives"] = [wall(w, lambda: w.set_joint_drives(drives)) for _ in range(total)]
        same = None
        if has_calls:
            out = torch.zeros(n_joints * capi.JOINT_STATE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
            ms["states_device"] = [events(lambda: w.joint_states_device(None, n_joints, out.data_ptr())) for _ in range(total)]
            ms["states_host"] = [wall(w, w.joint_states) for _ in range(total)]
            same = out.cpu().numpy().tobytes() == w.joint_states().tobytes()
            every = np.arange(n_drives, dtype=np.uint32)
            for tag, idx in (("all", every), ("1pct", np.ascontiguousarray(every[::100]))):
                dev_idx = torch.from_numpy(idx.view(np.int32).copy()).cuda()
                dev_targets = torch.full((len(idx),), 1.0, dtype=torch.float64, device="cuda")
                targets = np.full(len(idx), 1.0)
                ms["targets_device_" + tag] = [events(lambda: w.set_drive_targets_device(dev_idx.data_ptr(), dev_targets.data_ptr(), len(idx)))
                                               for _ in range(total)]
                ms["targets_host_" + tag] = [wall(w, lambda: w.set_drive_targets(idx, targets)) for _ in range(total)]
        w.step(bench.FRAME_TIME, args.substeps)
        finite = bool(np.isfinite(w.download()).all())
        w.set_stream(0)
    frame = statistics.median(ms["frame"][args.warmup:])
    own_tree = os.path.abspath(args.root) == os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    result = {"tree": "this checkout" if own_tree else "another checkout (--root)", "bodies": n, "joints": int(n_joints), "drives": int(n_drives), "substeps": args.substeps,
              "repeats": args.repeats, "warmup": args.warmup, "finite": finite, "states_device_equals_host": same}
    for name, values in ms.items():
        v = values[args.warmup:]
        result["ms_" + name] = {"median": statistics.median(v), "min": min(v), "max": max(v), "of_a_frame": statistics.median(v) / frame}
    if args.parent:
        with open(args.parent) as f:
            result["parent_commit"] = json.load(f)
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(result, what="scripts/joint_state_bench.py: joint states and drive targets on bench.py's joints scene; device "
                                        "variants by HIP events on the world's stream, host variants and downloads by wall time with the "
                                        "world synchronised; median [min, max] of %d after %d" % (args.repeats, args.warmup)), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
