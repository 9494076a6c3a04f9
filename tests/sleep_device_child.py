"""Child process of test_gpu_sleeping.py: the device variants of the calls that wake sleepers (xpbd_world_wake_bodies_device,
_set_external_wrench_device, _apply_impulses_device) and xpbd_world_sleep_state_device, driven from torch tensors on a torch
stream handed to the world with set_stream, beside the same sequence made with the host variants in a second world.  A process
of its own that imports torch first (as islands_device_child.py).  Writes both worlds' states after every edit to the .npz
named on the command line and prints one JSON line; the parent compares them."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from constraint_solver_amd import capi  # noqa: E402
import sleep_common as sc  # noqa: E402

QUICK = (0.1, 0.5, 5)


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).view(np.uint8).reshape(-1)).cuda()


def edits(w, bodies, device):
    """[(what it must wake, the call)]: body 1 of the stack 0-2 three ways, then the fixed slab 6."""
    force = bodies[1, 10:13].reshape(1, 3).copy()
    imp = capi.impulses([1], np.zeros((1, 3)))
    if not device:
        return [("stack", lambda: w.wake_bodies([1])),
                ("stack", lambda: w.set_external_wrench([1], force=force)),
                ("stack", lambda: w.apply_impulses(imp)),
                ("all", lambda: w.set_external_wrench([6], force=np.zeros((1, 3)))),
                ("all", lambda: w.wake_bodies())]
    keep = {"one": dev([1], np.uint32), "slab": dev([6], np.uint32), "force": dev(force, np.float64), "zero": dev(np.zeros(3), np.float64),
            "imp": dev(imp, capi.IMPULSE_DTYPE)}
    edits.keep = keep                                        # (the tensors outlive the calls)
    return [("stack", lambda: w.wake_bodies_device(keep["one"].data_ptr(), 1)),
            ("stack", lambda: w.set_external_wrench_device(keep["one"].data_ptr(), 1, keep["force"].data_ptr(), None)),
            ("stack", lambda: w.apply_impulses_device(keep["imp"].data_ptr(), 1)),
            ("all", lambda: w.set_external_wrench_device(keep["slab"].data_ptr(), 1, keep["zero"].data_ptr(), None)),
            ("all", lambda: w.wake_bodies_device(None, 0))]


def run(device, res, stream):
    tag = "device" if device else "host"
    w, _ = sc.crafted_world(QUICK)
    woke = {"stack": [], "all": []}
    if device:
        w.set_stream(stream.cuda_stream)
    for _ in range(12):
        w.step(sc.DT, sc.SUBSTEPS)
    bodies = w.download()
    for k, (what, call) in enumerate(edits(w, bodies, device)):
        call()
        w.step(sc.DT, sc.SUBSTEPS)
        if device:                                           # the device read-out first: nothing has waited for the step yet
            n = w.n
            d_asleep = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda")
            d_rest = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            d_group = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            d_counts = torch.full((4,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
            w.sleep_state_device(d_asleep.data_ptr(), d_rest.data_ptr(), d_group.data_ptr(), d_counts.data_ptr())
            res["%s_%d_dev_asleep" % (tag, k)] = d_asleep.cpu().numpy()
            res["%s_%d_dev_rest_frames" % (tag, k)] = d_rest.cpu().numpy().view(np.uint32)
            res["%s_%d_dev_group" % (tag, k)] = d_group.cpu().numpy().view(np.uint32)
            res["%s_%d_dev_counts" % (tag, k)] = d_counts.cpu().numpy().view(np.uint32)
        asleep, rest, group, counts = w.sleep_state()
        res["%s_%d_asleep" % (tag, k)], res["%s_%d_rest_frames" % (tag, k)], res["%s_%d_group" % (tag, k)] = asleep, rest, group
        res["%s_%d_counts" % (tag, k)] = np.array(counts, dtype=np.uint32)
        res["%s_%d_bodies" % (tag, k)] = w.download()
        woke[what].append(k)
        for _ in range(8):                                   # everything that can sleep is asleep again
            w.step(sc.DT, sc.SUBSTEPS)
    if device:
        w.set_stream(0)
    w.close()
    return len(woke["stack"]) + len(woke["all"]), woke


def main(out_path):
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    res = {}
    with torch.cuda.stream(stream):
        steps, woke = run(True, res, stream)
        run(False, res, stream)
    np.savez(out_path, **res)
    print(json.dumps({"steps": steps, "woke_stack": woke["stack"], "woke_all": woke["all"]}))


if __name__ == "__main__":
    main(sys.argv[1])
