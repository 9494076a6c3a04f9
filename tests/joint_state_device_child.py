"""Child process of test_gpu_joint_states.py: xpbd_world_joint_states_device and xpbd_world_set_drive_targets_device driven
from torch tensors on a torch stream handed to the world with set_stream.  A process of its own that imports torch first, so
that the library binds to the HIP runtime torch carries (as bench.py and islands_device_child.py do).  It makes the runs of
tests/joint_state_common.py with the device variants, writes what they leave to the .npz named on the command line and prints
one JSON line; the parent makes the same runs with the host variants and compares."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from constraint_solver_amd import capi  # noqa: E402
import joint_state_common as jc  # noqa: E402

RECORD = capi.JOINT_STATE_DTYPE.itemsize
KEEP = []                     # tensors handed to the library stay referenced until the process ends


def dev_u32(values):
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()
    KEEP.append(t)
    return t


def dev_f64(values):
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64).copy()).cuda()
    KEEP.append(t)
    return t


def device_states(w, joints, n, guard=0):
    """Records of one device call into a buffer pre-filled with 0x5A bytes, `guard` records of it before and behind the call's."""
    out = torch.full(((n + 2 * guard) * RECORD,), 0x5A, dtype=torch.uint8, device="cuda")
    KEEP.append(out)
    w.joint_states_device(None if joints is None else dev_u32(joints).data_ptr(), n, out.data_ptr() + guard * RECORD)
    return out.cpu().numpy().view(capi.JOINT_STATE_DTYPE)


def device_retarget(w, drives, targets):
    w.set_drive_targets_device(None if drives is None else dev_u32(drives).data_ptr(), dev_f64(targets).data_ptr(), len(targets))


def on_stream(w, stream):
    w.set_stream(stream.cuda_stream)
    return w


def states_runs(stream, res):
    w, scene = jc.stepped_world(jc.STATE_WORLDS[0], 0)
    with on_stream(w, stream):
        n = len(scene[2])
        res["states_device_all"] = device_states(w, None, n)
        res["states_host_all"] = w.joint_states()
        subset = np.array([n - 1, 3, 17, 3, 0], dtype=np.uint32)
        res["states_subset"], res["states_device_subset"], res["states_host_subset"] = subset, device_states(w, subset, len(subset)), w.joint_states(subset)
        outside = np.array([5, n, 9, 0xFFFFFFFF, 2], dtype=np.uint32)
        res["states_outside"], res["states_device_outside"] = outside, device_states(w, outside, len(outside), guard=1)
        w.set_stream(0)


def host_copy_run(stream, big, change):
    """Device retarget of every drive, then `change` re-stages the extras from the host copy; and a fresh world built from the
    state at that point with the new targets.  Returns the rows of both after RETARGET_THEN more frames."""
    bodies, sid, joints, lims, drvs, n_mech = jc.driven_scene(big, extra_bodies=1)
    targets = jc.new_targets(drvs)
    table = drvs.copy()
    table["target"] = targets
    with on_stream(jc.new_world(bodies, sid, joints, lims, drvs), stream) as w:
        for _ in range(jc.RETARGET_AT):
            w.step(jc.DT, jc.SUBSTEPS)
        device_retarget(w, None, targets)
        if change == "remove":                                        # an unrelated body leaves: a population change
            w.remove_bodies([n_mech - 1])
            sid = np.delete(sid, n_mech - 1)
            n_mech -= 1
        else:                                                         # a SLIDE limit on a slider that had none
            bare = [k for k in range(len(joints)) if joints["kind"][k] == capi.JOINT_SLIDER
                    and not ((lims["joint"] == k) & (lims["kind"] == capi.LIMIT_SLIDE)).any()]
            more = np.zeros(1, dtype=capi.JOINT_LIMIT_DTYPE)
            more["joint"], more["kind"], more["lower"], more["upper"] = bare[0], capi.LIMIT_SLIDE, -0.01, 0.01
            lims = np.concatenate([lims, more])
            w.set_joint_limits(lims)
        at_change = w.download()
        for _ in range(jc.RETARGET_THEN):
            w.step(jc.DT, jc.SUBSTEPS)
        kept = w.download()[:n_mech]
        w.set_stream(0)
    with jc.new_world(at_change, sid, joints, lims, table) as f:
        for _ in range(jc.RETARGET_THEN):
            f.step(jc.DT, jc.SUBSTEPS)
        return kept, f.download()[:n_mech]


def target_runs(stream, res):
    for big in (False, True):
        tag = "big_" if big else "small_"
        drvs = jc.driven_scene(False)[4]

        def retarget(w, drives, targets):
            w.set_stream(stream.cuda_stream)
            device_retarget(w, drives, targets)
            w.synchronize()
            w.set_stream(0)

        res[tag + "all"] = jc.retarget_run(retarget, big, None, jc.new_targets(drvs))
        res[tag + "some"] = jc.retarget_run(retarget, big, *jc.some_drives(drvs))
        drives, targets, _ = jc.invalid_list(drvs)
        res[tag + "invalid"] = jc.retarget_run(retarget, big, drives, targets)
        for change in ("remove", "slide"):
            res[tag + change + "_kept"], res[tag + change + "_fresh"] = host_copy_run(stream, big, change)


def sleeping_run(stream, res):
    w, drvs = jc.sleeping_world()
    with on_stream(w, stream):
        res["sleep_device"] = jc.wake_sequence(w, drvs, device_retarget)
        w.set_stream(0)


def loop_run(stream, res):
    """read state -> decide -> act, with no host copy inside the loop: the angle is read, the target is formed and written on
    the device, all on the world's stream."""
    rows, joints, lims, drvs = jc.loop_scene()
    with on_stream(jc.new_world(rows, np.zeros(len(rows), dtype=np.uint32), joints, lims, drvs), stream) as w:
        state = torch.zeros(RECORD, dtype=torch.uint8, device="cuda")
        for _ in range(jc.LOOP_FRAMES):
            w.joint_states_device(None, 1, state.data_ptr())
            angle = state.view(torch.float64)[2:3]
            target = jc.LOOP_GAIN * (jc.LOOP_GOAL - angle)
            KEEP.append(target)
            w.set_drive_targets_device(None, target.data_ptr(), 1)
            w.step(jc.DT, jc.SUBSTEPS)
        res["loop_rows"] = w.download()
        res["loop_state"] = w.joint_states()
        w.set_stream(0)


def main(out_path):
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    res = {}
    with torch.cuda.stream(stream):
        states_runs(stream, res)
        target_runs(stream, res)
        sleeping_run(stream, res)
        loop_run(stream, res)
    np.savez(out_path, **res)
    print(json.dumps({"runs": len(res)}))


if __name__ == "__main__":
    main(sys.argv[1])
