#!/usr/bin/env python3
"""Sliders and joint drives on bench.py's joints scene (262 144 unit boxes, 65 408 joints in chains of five, every fourth a
hinge; SAT, 20 substeps): one JSON line per run, timed with events on the world's stream.

  --config none     no drives: the pair-solve kernels as every jointed world without drives runs them
  --config drives   an XPBD_DRIVE_ANGULAR_VELOCITY drive on every joint that can take one (the hinges)
--root <tree> imports the package (and bench.py's scene) of another checkout, built there: the A/B of --config none against
the parent commit.  Run the two trees alternately in one session, and the parent against itself first: the spread of its
--runs runs is the yardstick.  Every run is a world of its own: pre-roll (bench.py's), warm-up, then --frames timed frames."""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=["none", "drives"], default="none")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--joints", type=int, default=65536)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--speed", type=float, default=1.0, help="rad/s of every drive")
    ap.add_argument("--seed", type=int, default=1)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import numpy as np
    import torch
    import bench
    from constraint_solver_amd import capi

    kind = capi.SCENE_BOXES_DROP
    n = args.bodies
    grid_w = bench.scene_grid_width(capi, kind, n, n)
    state, sid = capi.scene_generate(kind, args.seed, n, grid_w=grid_w)
    joints = bench.chain_joints(capi, np, args.joints, n, 2.0, grid_w, state=state)
    drives = None
    if args.config == "drives":
        hinges = np.nonzero(joints["kind"] == capi.JOINT_HINGE)[0]
        drives = np.zeros(len(hinges), dtype=capi.JOINT_DRIVE_DTYPE)
        drives["joint"], drives["kind"], drives["target"], drives["max_force"] = hinges, capi.DRIVE_ANGULAR_VELOCITY, args.speed, np.inf
        for side in "ab":                                  # a unit reference perpendicular to each (unit) axis
            axis = joints["axis_" + side][hinges]
            ref = np.cross(axis, np.where(np.abs(axis[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]]))
            drives["ref_" + side] = ref / np.linalg.norm(ref, axis=1, keepdims=True)
    stream = torch.cuda.current_stream()
    for run in range(args.runs):
        with capi.World(mode=capi.MODE_CONTACTS) as w:
            w.set_polytopes(capi.scene_polytopes(kind))
            w.set_contact_pad(0.02)
            w.set_narrowphase(capi.NARROWPHASE_SAT)
            w.upload(state, sid)
            w.set_joints(joints)
            if drives is not None:
                w.set_joint_drives(drives)
            w.set_stream(stream.cuda_stream)
            for _ in range(bench.PREROLL["boxes-drop"] + args.warmup):
                w.step(bench.FRAME_TIME, args.substeps)
            w.contact_stats()
            _, device_ms = bench.timed_frames(lambda: w.step(bench.FRAME_TIME, args.substeps), stream, args.frames)
            pairs, touching, points = w.contact_stats()
            end = w.download()
        print(json.dumps({"config": args.config, "root": os.path.abspath(args.root), "run": run, "bodies": n, "joints": int(len(joints)),
                          "drives": 0 if drives is None else int(len(drives)), "substeps": args.substeps, "frames": args.frames,
                          "ms_per_frame": device_ms / args.frames, "body_substeps_per_s": n * args.substeps * args.frames / (device_ms * 1e-3),
                          "touching_per_substep": touching / (args.frames * args.substeps), "finite": bool(np.isfinite(end).all()),
                          "state_crc": int(np.bitwise_xor.reduce(end.view(np.uint64).ravel()))}), flush=True)


if __name__ == "__main__":
    main()
