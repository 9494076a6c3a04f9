#!/usr/bin/env python3
"""Host wall time per call of set_joint_drives and set_joint_limits on the joints scene of scripts/joint_drives_bench.py
(262 144 boxes, 65 408 joints, one ANGULAR_VELOCITY drive / one HINGE limit per hinge): median of 20 calls after 3 warm-up
calls, one JSON line (profiles/joint_setters_host_time.json).  --root <tree> imports the package (and bench.py's scene) of
another checkout, built there: run the two trees in alternating processes in one session."""
import argparse
import json
import os
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--tag", default="this", help="names the tree in the output")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch  # noqa: F401
    import bench
    from constraint_solver_amd import capi

    kind, n = capi.SCENE_BOXES_DROP, 262144
    grid_w = bench.scene_grid_width(capi, kind, n, n)
    state, sid = capi.scene_generate(kind, 1, n, grid_w=grid_w)
    joints = bench.chain_joints(capi, np, 65536, n, 2.0, grid_w, state=state)
    hinges = np.nonzero(joints["kind"] == capi.JOINT_HINGE)[0]
    drives = np.zeros(len(hinges), dtype=capi.JOINT_DRIVE_DTYPE)
    drives["joint"], drives["kind"], drives["target"], drives["max_force"] = hinges, capi.DRIVE_ANGULAR_VELOCITY, 1.0, np.inf
    lims = np.zeros(len(hinges), dtype=capi.JOINT_LIMIT_DTYPE)
    lims["joint"], lims["kind"], lims["lower"], lims["upper"] = hinges, capi.LIMIT_HINGE, -1.0, 1.0
    for side in "ab":
        axis = joints["axis_" + side][hinges]
        ref = np.cross(axis, np.where(np.abs(axis[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]]))
        ref = ref / np.linalg.norm(ref, axis=1, keepdims=True)
        drives["ref_" + side] = ref
        lims["ref_" + side] = ref
    out = {"tag": args.tag, "bodies": n, "joints": int(len(joints)), "drives": int(len(drives)), "limits": int(len(lims))}
    with capi.World(mode=capi.MODE_CONTACTS) as w:
        w.set_polytopes(capi.scene_polytopes(kind))
        w.set_narrowphase(capi.NARROWPHASE_SAT)
        w.upload(state, sid)
        w.set_joints(joints)
        for name, call, value in [("set_joint_drives", w.set_joint_drives, drives), ("set_joint_limits", w.set_joint_limits, lims)]:
            ms = []
            for k in range(23):
                t0 = time.perf_counter()
                call(value)
                ms.append((time.perf_counter() - t0) * 1e3)
            ms = ms[3:]
            out[name + "_ms"] = {"median": statistics.median(ms), "min": min(ms), "max": max(ms), "calls": ms}
        w.step(1.0 / 60.0, 20)
        out["finite"] = bool(np.isfinite(w.download()).all())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
