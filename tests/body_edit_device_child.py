"""Child process of test_gpu_body_edits.py: the DEVICE variants of the body edits driven from torch tensors on a torch stream
handed to the world with set_stream.  A process of its own that imports torch first, so that the library binds to the HIP
runtime torch carries (as bench.py and test_gpu_raycast.py's child do).  Writes its results to the .npz named on the command
line; the parent compares them with the host variants."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from constraint_solver_amd import capi  # noqa: E402
import body_edit_common as bc  # noqa: E402


def device_bytes(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to("cuda")


def main(out_path):
    torch.cuda.set_device(0)
    kind = capi.SCENE_MIXED_DROP
    bodies, sid = bc.scene(kind)
    stream = torch.cuda.Stream()
    res = {}
    with torch.cuda.stream(stream):
        # impulses: the pre-sorted list, then a list whose only entry names body == body count (skipped)
        w = bc.world(kind, bodies, sid)
        w.set_stream(stream.cuda_stream)
        entries = bc.presorted(bc.shuffled(bc.impulse_list(bodies, 11), 12))
        dev = device_bytes(entries)
        w.apply_impulses_device(dev.data_ptr(), entries.size)
        res["impulses_device"] = w.download()
        beyond = capi.impulses(bc.N, [1.0, 2.0, 3.0], point=[0.0, 0.0, 0.0], angular_impulse=[1.0, 1.0, 1.0])
        dev_beyond = device_bytes(beyond)
        w.apply_impulses_device(dev_beyond.data_ptr(), 1)
        idx_beyond = device_bytes(np.array([bc.N], dtype=np.uint32))
        xyz = device_bytes(np.array([[5.0, 6.0, 7.0]]))
        w.set_external_wrench_device(idx_beyond.data_ptr(), 1, xyz.data_ptr(), xyz.data_ptr())
        res["beyond"] = w.download()
        w.set_stream(0)
        w.close()

        # wrench from tensors, then step at once: nothing waits between the edit and the step
        w = bc.world(kind, bodies, sid)
        w.set_stream(stream.cuda_stream)
        force, torque = bc.wrench_values(21)
        idx = np.array([129, 0, 64, 63, 17, 100], dtype=np.uint32)
        dev_idx = torch.from_numpy(idx.astype(np.int32)).to("cuda")
        dev_force = torch.from_numpy(force[idx]).to("cuda") * 1.0        # a tensor the stream has just computed
        dev_torque = torch.from_numpy(torque[idx]).to("cuda") * 1.0
        w.set_external_wrench_device(dev_idx.data_ptr(), idx.size, dev_force.data_ptr(), dev_torque.data_ptr())
        w.step(bc.DT, bc.SUBSTEPS)
        dev_all = torch.from_numpy(force).to("cuda") * 1.0
        w.set_external_wrench_device(0, bc.N, dev_all.data_ptr(), 0)     # the indices == NULL form, force only
        for _ in range(bc.FRAMES - 1):
            w.step(bc.DT, bc.SUBSTEPS)
        res["wrench_bodies"], res["wrench_contacts"] = w.download(), w.contacts()
        w.set_stream(0)
        w.close()
    np.savez(out_path, **res)


if __name__ == "__main__":
    main(sys.argv[1])
