"""Child process of test_gpu_mass_edit.py: xpbd_world_set_mass_properties_device driven from torch tensors on a torch stream handed
to the world with set_stream.  A process of its own that imports torch first, so that the library binds to the HIP runtime torch
carries (as bench.py and kinematic_device_child.py do).  It makes the runs of tests/mass_edit_common.py with the device variant,
writes what they leave to the .npz named on the command line and prints one JSON line; the parent makes the same runs with the
host variant, or asks the model, and compares."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from constraint_solver_amd import capi  # noqa: E402
import mass_edit_common as mc  # noqa: E402
import mass_edit_model as mm  # noqa: E402

KEEP = []                     # tensors handed to the library stay referenced until the process ends


def dev_u32(values):
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()
    KEEP.append(t)
    return t


def dev_f64(values):
    t = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64).copy()).cuda()
    KEEP.append(t)
    return t


def device_edit_on(stream, wait=True):
    def edit(w, indices, rows, flags=mm.INVERSE):
        rows = np.asarray(rows, dtype=np.float64).reshape(-1, 13)
        w.set_stream(stream.cuda_stream)
        w.set_mass_properties_device(None if indices is None else dev_u32(indices).data_ptr(), len(rows), dev_f64(rows).data_ptr(), flags)
        if wait:
            w.synchronize()
    return edit


def skipped_entries(edit):
    """A list with every kind of entry the kernel skips among good ones, on the DIRECT scene: (download before, after, indices,
    rows).  Body 2 is fixed and kinematic: the entry that would give it mass is skipped, the one that only moves its centre of
    mass is not the same body's (the same index twice is unspecified), so body 3, also kinematic, takes the legal row."""
    bodies, sid = mc.direct_scene()
    bodies[[2, 3], 0:10] = 0.0
    rows = mc.trip_rows(9, seed=6500)
    idx = np.array([0, 1, 2, 3, 40, 0xFFFFFFFF, 6, 7, 8], dtype=np.uint32)
    rows[0, 0:10] = 0.5                                                   # (trip_rows makes row 0 fixed and row 1 massless)
    rows[1, 0] = 0.25
    rows[3, 0:10] = 0.0                                                   # legal for kinematic body 3
    rows[6, 5] = np.nan
    rows[7, 0] = -0.5
    with mc.new_world(bodies, sid) as w:
        w.set_kinematics(capi.kinematics([2, 3], capi.KINEMATIC_POSE, bodies[[2, 3], 31:34], [mc.IDENT, mc.IDENT]))
        before = w.download()
        edit(w, idx, rows, mm.INVERSE)
        return before, w.download(), idx, rows


def no_wait_run(stream, wait):
    """The block scene: a device edit of three bodies immediately followed by xpbd_world_step on the same stream."""
    bodies, sid = mc.block_scene()
    with mc.new_world(bodies, sid) as w:
        mc.block_settings(w)
        for _ in range(mc.PRE_FRAMES):
            w.step(mc.DT, mc.SUBSTEPS)
        edits = mc.block_edits(w.get_mass_properties())                   # (waits: the stream changes hands with nothing queued)
        w.set_stream(stream.cuda_stream)
        for idx, rows, flags in edits:
            w.set_mass_properties_device(dev_u32(idx).data_ptr(), len(rows), dev_f64(rows).data_ptr(), flags)
        if wait:
            w.synchronize()
        for _ in range(mc.POST_FRAMES):
            w.step(mc.DT, mc.SUBSTEPS)
        out = w.download()
        w.set_stream(0)
        return out


def main(out_path):
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    res = {}
    with torch.cuda.stream(stream):
        edit = device_edit_on(stream)
        for which in mc.TRIP_LISTS:
            _, _, after, got, _ = mc.trip_run(edit, which)
            res["trip_" + which], res["trip_get_" + which] = after, got
        _, res["direct"] = mc.direct_run(edit)
        res["direct_singular_before"], res["direct_singular"] = mc.direct_run(edit, singular=True)
        _, _, res["keep"], res["keep_frames"], _ = mc.keep_run(edit)
        res["skip_before"], res["skip_after"], res["skip_idx"], res["skip_rows"] = skipped_entries(edit)
        res["no_wait"] = no_wait_run(stream, wait=False)
        res["waited"] = no_wait_run(stream, wait=True)
    np.savez(out_path, **res)
    print(json.dumps({"runs": len(res)}))


if __name__ == "__main__":
    main(sys.argv[1])
