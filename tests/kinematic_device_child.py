"""Child process of test_gpu_kinematic.py: xpbd_world_set_kinematic_targets_device driven from torch tensors on a torch stream
handed to the world with set_stream.  A process of its own that imports torch first, so that the library binds to the HIP
runtime torch carries (as bench.py and joint_state_device_child.py do).  It makes the runs of tests/kinematic_common.py with the
device variant, writes what they leave to the .npz named on the command line and prints one JSON line; the parent makes the
same runs with the host variant and compares."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from constraint_solver_amd import capi  # noqa: E402
import kinematic_common as kc  # noqa: E402

KEEP = []                     # tensors handed to the library stay referenced until the process ends


def dev_u32(values):
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()
    KEEP.append(t)
    return t


def dev_f64(values):
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64).copy()).cuda()
    KEEP.append(t)
    return t


def device_retarget_on(stream):
    def retarget(w, tbl, entries, rows):
        w.set_stream(stream.cuda_stream)
        w.set_kinematic_targets_device(None if entries is None else dev_u32(entries).data_ptr(), dev_f64(rows).data_ptr(), len(rows))
        w.synchronize()
        w.set_stream(0)
    return retarget


def host_copy_run(stream):
    """Device retarget of every entry, then a population change re-stages the table from the host copy; and a fresh world built
    from the state at that point with the new rows.  Returns the rows of both after RETARGET_THEN more frames."""
    bodies, sid, tbl = kc.retarget_scene()
    rows = kc.new_rows()
    gone = kc.N_PLATFORMS + 1                                         # a rider leaves: no entry changes its body
    with kc.new_world(bodies, sid) as w:
        w.set_stream(stream.cuda_stream)
        w.set_kinematics(kc.to_capi(tbl))
        for _ in range(kc.RETARGET_AT):
            w.step(kc.DT, kc.RETARGET_SUBSTEPS)
        w.set_kinematic_targets_device(None, dev_f64(rows).data_ptr(), len(rows))
        w.remove_bodies([gone])
        at_change = w.download()
        for _ in range(kc.RETARGET_THEN):
            w.step(kc.DT, kc.RETARGET_SUBSTEPS)
        kept = w.download()
        w.set_stream(0)
    fresh_tbl = tbl.copy()
    fresh_tbl["linear"], fresh_tbl["angular"] = rows[:, 0:3], rows[:, 3:7]
    with kc.new_world(at_change, np.delete(sid, gone)) as f:
        f.set_kinematics(kc.to_capi(fresh_tbl))
        for _ in range(kc.RETARGET_THEN):
            f.step(kc.DT, kc.RETARGET_SUBSTEPS)
        return kept, f.download()


def main(out_path):
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    res = {}
    with torch.cuda.stream(stream):
        retarget = device_retarget_on(stream)
        res["all"] = kc.retarget_run(retarget, None, kc.new_rows())
        res["some"] = kc.retarget_run(retarget, *kc.some_entries())
        entries, rows, _ = kc.invalid_list()
        res["invalid"] = kc.retarget_run(retarget, entries, rows)
        res["remove_kept"], res["remove_fresh"] = host_copy_run(stream)
    np.savez(out_path, **res)
    print(json.dumps({"runs": len(res)}))


if __name__ == "__main__":
    main(sys.argv[1])
