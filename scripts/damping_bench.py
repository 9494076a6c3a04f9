#!/usr/bin/env python3
"""Damping on bench.py's two big scenes (262 144 unit boxes, SAT, 20 substeps): one JSON line, the whole result in --out.

  --scene pile     the boxes dropped as a pile and pre-rolled to rest (bench.py's headline scene)
  --scene joints   the boxes on the grid with 65 408 joints in chains of five, every fourth a hinge (bench.py's configs[4])

After bench.py's pre-roll, median [min, max] of --repeats after --warmup, HIP events on the world's stream (a torch stream of this
script's own, handed to the world, so that an event pair brackets exactly the kernels enqueued between them):
  ms_frame_plain           one xpbd_world_step of a world that never called the setters: the fused schedule
  ms_frame_drag            drag --drag 1/s on every body: the unfused schedule plus k_body_damping behind every substep
  ms_frame_joint_dampers   (joints) dampers --mu 1/s, linear and angular, on every hinge: k_joint_damping as well
  ms_frame_plain_again     both tables cleared again: the launches of ms_frame_plain
  ms_substep_plain / _drag / _joint_dampers   one xpbd_world_contacts_substep (the split API runs the unfused substep either way),
                           so ms_pass_drag and ms_pass_joint_dampers, the differences of the medians, are the pass's own time
  sleeping (pile, --sleeping): with sleeping on, thresholds 1.5 x the 99.9th percentile of a 30-frame speed census of the undamped
                           pile (as scripts/sleeping_bench.py) and frames_to_sleep 30, for every drag of --sleep-drags: the share of
                           bodies asleep after --sleep-frames frames and the frame time then
--root <tree> imports the package (and bench.py's scene) of another checkout, built there; a tree without the new calls is timed
for ms_frame_plain alone.  --parent <json ...>: the --out files of such runs of the parent commit, alternating with runs of this
tree; their ms_frame_plain is stored beside this tree's figures and the ranges are compared, no difference is claimed."""
import argparse
import json
import os
import statistics
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--scene", default="pile", choices=["pile", "joints"])
    ap.add_argument("--bodies", type=int, default=262144)
    ap.add_argument("--joints", type=int, default=65536)
    ap.add_argument("--substeps", type=int, default=20)
    ap.add_argument("--preroll", type=int, default=-1, help="frames before anything is timed (default: bench.py's for the scene)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--drag", type=float, default=1.0)
    ap.add_argument("--mu", type=float, default=10.0)
    ap.add_argument("--sleeping", action="store_true")
    ap.add_argument("--sleep-drags", type=float, nargs="*", default=[0.0, 1.0, 5.0, 20.0])
    ap.add_argument("--sleep-frames", type=int, default=90)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--parent", nargs="*", default=[])
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
    joints = None
    if args.scene == "pile":
        state, sid = capi.scene_pile(kind, args.seed, n, 1.8, 4)
        preroll = bench.PREROLL_PILE
    else:
        grid_w = bench.scene_grid_width(capi, kind, n, n)
        state, sid = capi.scene_generate(kind, args.seed, n, grid_w=grid_w)
        joints = bench.chain_joints(capi, np, args.joints, n, 2.0, grid_w, state=state)
        preroll = bench.PREROLL["boxes-drop"]
    preroll = args.preroll if args.preroll >= 0 else preroll
    has_calls = hasattr(capi.World, "set_damping")
    stream = torch.cuda.Stream()          # a stream of its own: the events are then ordered with the world's kernels, not with the host
    total = args.warmup + args.repeats
    h = bench.FRAME_TIME / args.substeps

    def events(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        call()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    def new_world():
        w = capi.World(mode=capi.MODE_CONTACTS)
        w.set_polytopes(capi.scene_polytopes(kind))
        w.set_contact_pad(0.02)
        w.set_narrowphase(capi.NARROWPHASE_SAT)
        w.upload(state, sid)
        if joints is not None:
            w.set_joints(joints)
        w.set_stream(stream.cuda_stream)
        for _ in range(preroll):
            w.step(bench.FRAME_TIME, args.substeps)
        return w

    ms, sleeping = {}, []
    with new_world() as w:
        frame = lambda: w.step(bench.FRAME_TIME, args.substeps)      # noqa: E731
        ms["frame_plain"] = [events(frame) for _ in range(total)]
        if has_calls:
            drag = capi.body_damping(n, linear=args.drag, angular=args.drag)
            hinges = np.nonzero(joints["kind"] == capi.JOINT_HINGE)[0] if joints is not None else np.zeros(0, dtype=np.uint32)
            dampers = capi.joint_damping(hinges, args.mu, args.mu)

            def substeps_of(label):
                w.contacts_begin(bench.FRAME_TIME)
                ms["substep_" + label] = [events(lambda: w.contacts_substep(h)) for _ in range(total)]

            substeps_of("plain")
            w.set_damping(drag)
            ms["frame_drag"] = [events(frame) for _ in range(total)]
            substeps_of("drag")
            w.set_damping(None)
            if len(hinges):
                w.set_joint_damping(dampers)
                ms["frame_joint_dampers"] = [events(frame) for _ in range(total)]
                substeps_of("joint_dampers")
                w.set_joint_damping(None)
            ms["frame_plain_again"] = [events(frame) for _ in range(total)]
        finite = bool(np.isfinite(w.download()).all())
        w.set_stream(0)

    if has_calls and args.sleeping:
        # the census of scripts/sleeping_bench.py: every body's peak speeds over 30 frames of the undamped world without sleeping
        with new_world() as w:
            peak_v, peak_w = np.zeros(n), np.zeros(n)
            for _ in range(30):
                w.step(bench.FRAME_TIME, args.substeps)
                b = w.download()
                peak_v = np.maximum(peak_v, np.linalg.norm(b[:, 22:25], axis=1))
                peak_w = np.maximum(peak_w, np.linalg.norm(b[:, 25:28], axis=1))
            w.set_stream(0)
        thresholds = (1.5 * float(np.percentile(peak_v, 99.9)), 1.5 * float(np.percentile(peak_w, 99.9)))
        for c in args.sleep_drags:
            with new_world() as w:
                w.set_contact_report(True)
                w.set_sleeping(thresholds[0], thresholds[1], 30)
                if c > 0.0:
                    w.set_damping(capi.body_damping(n, linear=c, angular=c))
                for _ in range(args.sleep_frames):
                    w.step(bench.FRAME_TIME, args.substeps)
                asleep = w.sleep_state()[0]
                b = w.download()
                times = [events(lambda: w.step(bench.FRAME_TIME, args.substeps)) for _ in range(total)][args.warmup:]
                sleeping.append({"drag": c, "asleep_share": float(np.count_nonzero(asleep)) / n, "frames": args.sleep_frames,
                                 "speed_p50": float(np.percentile(np.linalg.norm(b[:, 22:25], axis=1), 50)),
                                 "speed_p99_9": float(np.percentile(np.linalg.norm(b[:, 22:25], axis=1), 99.9)),
                                 "ms_frame_then": {"median": statistics.median(times), "min": min(times), "max": max(times)}})
                w.set_stream(0)

    own_tree = os.path.abspath(args.root) == os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    result = {"tree": "this checkout" if own_tree else "another checkout (--root)", "scene": args.scene, "bodies": n,
              "joints": 0 if joints is None else int(len(joints)), "substeps": args.substeps, "repeats": args.repeats, "warmup": args.warmup,
              "drag": args.drag, "mu": args.mu, "finite": finite}
    base = statistics.median(ms["frame_plain"][args.warmup:])
    for name, values in ms.items():
        v = values[args.warmup:]
        entry = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        if name.startswith("frame"):
            entry["of_frame_plain"] = entry["median"] / base
        result["ms_" + name] = entry
    for label in ("drag", "joint_dampers"):
        if "ms_substep_" + label in result:
            result["ms_pass_" + label] = result["ms_substep_" + label]["median"] - result["ms_substep_plain"]["median"]
    if sleeping:
        result["sleeping"] = {"thresholds": thresholds, "frames_to_sleep": 30, "runs": sleeping}
    parents = []
    for path in args.parent:
        with open(path) as f:
            parents.append(json.load(f)["ms_frame_plain"])
    if parents:
        result["parent_commit_ms_frame_plain"] = parents
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(result, what="scripts/damping_bench.py: damping on bench.py's settled pile / joints scene; HIP events on the world's stream; "
                                        "median [min, max] of %d after %d" % (args.repeats, args.warmup)), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
