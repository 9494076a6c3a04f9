"""Child process of test_gpu_sensors.py: xpbd_world_sensor_overlaps_device driven from torch tensors on a torch stream handed to
the world with set_stream.  A process of its own that imports torch first, so that the library binds to the HIP runtime torch
carries (as islands_device_child.py does).  Writes its arrays to the .npz named on the command line and prints one JSON line; the
parent compares the device call's outputs with the host call's."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from constraint_solver_amd import capi  # noqa: E402
import sensor_common as sc  # noqa: E402

SHORT_CAP = 7
FILL = 0x5A5A5A5A


def device_call(w, cap):
    """(sensors, offsets, hits) of one device call into tensors pre-filled with 0x5A bytes."""
    k = w.sensor_count()
    sensors = torch.full((k,), FILL, dtype=torch.int32, device="cuda")
    offsets = torch.full((k + 1,), FILL, dtype=torch.int32, device="cuda")
    hits = torch.full((max(cap, 1) * 2,), FILL, dtype=torch.int32, device="cuda")
    w.sensor_overlaps_device(sensors.data_ptr(), offsets.data_ptr(), hits.data_ptr() if cap else None, cap)
    return sensors, offsets, hits


def to_numpy(t, dtype=np.uint32):
    return t.cpu().numpy().view(dtype)


def main(out_path):
    torch.cuda.set_device(0)
    stream = torch.cuda.Stream()
    res = {}
    with torch.cuda.stream(stream):
        w, is_sensor = sc.occupancy_world()
        w.set_stream(stream.cuda_stream)
        w.step(sc.DT, sc.OCC_SUBSTEPS)
        # the device call first: it is then the one that compacts the frame's keys and builds the sensor list
        room = 4 * w.n
        sensors, offsets, hits = device_call(w, room)
        res["device_sensors"], res["device_offsets"] = to_numpy(sensors), to_numpy(offsets)
        res["device_hits"] = to_numpy(hits, capi.SENSOR_HIT_DTYPE)
        res["host_sensors"], res["host_offsets"], res["host_hits"] = w.sensor_overlaps()
        res["pairs"] = w.pair_contacts(points=False)[0]
        sensors, offsets, hits = device_call(w, SHORT_CAP)
        res["short_offsets"], res["short_hits"] = to_numpy(offsets), to_numpy(hits, capi.SENSOR_HIT_DTYPE)
        # "who is in the zone" without leaving the device: the first big box's occupants, cut out of the hits by its two offsets
        sensors, offsets, hits = device_call(w, room)
        k = int(np.flatnonzero(res["host_sensors"] == sc.CLUMP)[0])
        inside = hits.view(-1, 2)[:, 0].long()
        lo, hi = offsets[k].long(), offsets[k + 1].long()
        at = torch.arange(room, device="cuda")
        res["zone"] = inside[(at >= lo) & (at < hi)].cpu().numpy().astype(np.uint32)
        w.set_stream(0)
        w.close()
    np.savez(out_path, **res)
    print(json.dumps({"short_cap": SHORT_CAP, "total": int(res["host_offsets"][-1]), "fill": FILL}))


if __name__ == "__main__":
    main(sys.argv[1])
