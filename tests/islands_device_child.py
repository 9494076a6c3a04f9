"""Child process of test_gpu_islands.py: xpbd_world_islands_device driven from torch tensors on a torch stream handed to the
world with set_stream.  A process of its own that imports torch first, so that the library binds to the HIP runtime torch
carries (as bench.py and population_device_child.py do).  Writes its arrays to the .npz named on the command line and prints
one JSON line; the parent compares the device call's outputs with the host call's."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from constraint_solver_amd import capi  # noqa: E402
import islands_common as ic  # noqa: E402

SHORT_CAP = 5
REST_SPEED2 = 0.05
RECORD_BYTES = capi.ISLAND_DTYPE.itemsize


def device_call(w, flags, cap, want_island_of=True, want_records=True):
    """(total, island_of, records) of one device call into tensors pre-filled with 0x5A bytes."""
    island_of = torch.full((w.n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    records = torch.full((max(cap, 1) * RECORD_BYTES,), 0x5A, dtype=torch.uint8, device="cuda")
    total = torch.full((1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    w.islands_device(flags, island_of.data_ptr() if want_island_of else None, records.data_ptr() if want_records else None,
                     cap if want_records else 0, total.data_ptr())
    return total, island_of, records


def to_records(t):
    return t.cpu().numpy().view(capi.ISLAND_DTYPE)


def main(out_path):
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    res, verdict = {}, {"short_cap": SHORT_CAP, "rest_speed2": REST_SPEED2}
    with torch.cuda.stream(stream):
        w, _ = ic.drop_world(fixed=(5, 200))
        w.set_stream(stream.cuda_stream)
        for _ in range(60):
            w.step(ic.DT, 10)
        n = w.n
        # the device call first: it is then the one that compacts the frame's keys, before any report call has waited
        first = device_call(w, 0, n)
        for flags in (0, capi.ISLANDS_NO_JOINTS, capi.ISLANDS_NO_CONTACTS):
            tag = "f%d_" % flags
            total, island_of, records = first if flags == 0 else device_call(w, flags, n)
            res[tag + "device_total"] = total.cpu().numpy().view(np.uint32)[0]
            res[tag + "device_island_of"] = island_of.cpu().numpy().view(np.uint32)
            res[tag + "device_records"] = to_records(records)
            host_of, host_records = w.islands(flags)
            res[tag + "host_total"], res[tag + "host_island_of"], res[tag + "host_records"] = np.uint32(len(host_records)), host_of, host_records
        res["host_total"], res["host_island_of"], res["host_records"] = res["f0_host_total"], res["f0_host_island_of"], res["f0_host_records"]
        verdict["total"] = int(res["host_total"])

        total, island_of, records = device_call(w, 0, SHORT_CAP)
        res["short_total"] = total.cpu().numpy().view(np.uint32)[0]
        res["short_island_of"], res["short_records"] = island_of.cpu().numpy().view(np.uint32), to_records(records)
        total, _, _ = device_call(w, 0, 0, want_island_of=False, want_records=False)
        res["count_only_total"] = total.cpu().numpy().view(np.uint32)[0]

        # "remove every island that has come to rest", with no host round trip between the islands and the removal
        total, island_of, records = device_call(w, 0, n)
        rec = records.view(torch.float64).view(n, RECORD_BYTES // 8)
        resting = (rec[:, 3] < REST_SPEED2) & (rec[:, 4] < REST_SPEED2) & (torch.arange(n, device="cuda") < total[0])
        member = island_of != -1                                                   # XPBD_ISLAND_NONE: a fixed body
        flags = (member & resting[torch.where(member, island_of, torch.zeros_like(island_of)).long()]).to(torch.uint8)
        dev_map = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        w.remove_bodies_device(flags.data_ptr(), dev_map.data_ptr())
        res["removal_map"] = dev_map.cpu().numpy().view(np.uint32)
        res["after_removal_count"] = np.uint32(w.n)
        w.set_stream(0)
        w.close()
    np.savez(out_path, **res)
    print(json.dumps(verdict))


if __name__ == "__main__":
    main(sys.argv[1])
