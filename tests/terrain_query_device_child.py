"""Child process of tests/test_gpu_terrain_queries.py: the device variants of the ray casts, sweeps and overlap queries with
XPBD_QUERY_TERRAIN, with torch tensors on a torch stream handed to the world with set_stream.  torch is imported first, so that
the library binds to the HIP runtime torch carries (as in bench.py).  Prints one JSON line of verdicts."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from constraint_solver_amd import capi  # noqa: E402
import test_gpu_terrain_queries as t  # noqa: E402

GUARD = 16
T, BRUTE = capi.QUERY_TERRAIN, 1


def main():
    torch.cuda.set_device(0)
    bodies, sid = t.pile(capi, t.BOXES, 96, 3, 4.0, 3.0)
    w = t.world(t.PILE_TERRAIN, t.BOXES, bodies, sid)
    for _ in range(10):
        w.step(t.DT, 6)
    state = w.download()
    rng = np.random.default_rng(77)
    rays = t.pile_rays(1024, 8)
    sweeps = t.terrain_sweeps(rng, 256, 1)
    k = 192
    _, queries = t.overlap_volumes(rng, k)
    groups = np.zeros(len(state), dtype=capi.COLLISION_FILTER_DTYPE)
    groups["group"], groups["mask"] = 1 << (np.arange(len(state)) % 3), 0xFFFFFFFF
    w.set_collision_filters(groups)
    host = {"rays": w.raycast(rays, T), "rays_masked": w.raycast(rays, T, mask=2), "rays_plain": w.raycast(rays), "sweeps": w.sweep(sweeps, T),
            "sweeps_plain": w.sweep(sweeps), "overlaps": w.overlap(queries, T), "overlaps_plain": w.overlap(queries)}
    res = {"terrain_seen": bool(all((host[name]["body"] == capi.HIT_TERRAIN).sum() > 20 for name in ("rays", "sweeps")) and
                                (host["overlaps"][1]["body"] == capi.HIT_TERRAIN).sum() > 20)}
    stream = torch.cuda.Stream()
    w.set_stream(stream.cuda_stream)
    guard = True

    def records(batch, size, call):
        """The device call on tensors of the batch and of len(batch) + GUARD records of `size` bytes; the raw bytes back."""
        nonlocal guard
        dev_in = torch.from_numpy(batch.view(np.uint8).copy()).to("cuda")
        dev_out = torch.full(((len(batch) + GUARD) * size,), 0xEE, dtype=torch.uint8, device="cuda")
        call(dev_in.data_ptr(), dev_out.data_ptr())
        raw = dev_out.cpu().numpy()                             # (the copy is ordered after the query on the same stream)
        guard = guard and bool((raw[len(batch) * size:] == 0xEE).all())
        return raw[:len(batch) * size].tobytes()

    def overlaps(flags, cap):
        nonlocal guard
        dev_q = torch.from_numpy(queries.view(np.uint8).copy()).to("cuda")
        dev_offsets = torch.full((k + 1 + GUARD,), 0x6EEEEEEE, dtype=torch.int32, device="cuda")
        dev_hits = torch.full(((cap + GUARD) * 16,), 0xEE, dtype=torch.uint8, device="cuda")
        w.overlap_device(dev_q.data_ptr(), k, dev_offsets.data_ptr(), dev_hits.data_ptr() if cap else 0, cap, flags)
        offsets, raw = dev_offsets.cpu().numpy(), dev_hits.cpu().numpy()
        guard = guard and bool((offsets[k + 1:] == 0x6EEEEEEE).all()) and bool((raw[cap * 16:] == 0xEE).all())
        return offsets[:k + 1].astype(np.uint32), raw[:cap * 16].tobytes()

    with torch.cuda.stream(stream):
        res["rays"] = records(rays, 64, lambda i, o: w.raycast_device(i, len(rays), o, T)) == host["rays"].tobytes()
        res["rays_brute"] = records(rays, 64, lambda i, o: w.raycast_device(i, len(rays), o, T | BRUTE)) == host["rays"].tobytes()
        res["rays_masked"] = records(rays, 64, lambda i, o: w.raycast_device(i, len(rays), o, T, mask=2)) == host["rays_masked"].tobytes()
        res["rays_plain"] = records(rays, 64, lambda i, o: w.raycast_device(i, len(rays), o, 0)) == host["rays_plain"].tobytes()
        res["sweeps"] = records(sweeps, 72, lambda i, o: w.sweep_device(i, len(sweeps), o, T)) == host["sweeps"].tobytes()
        res["sweeps_brute"] = records(sweeps, 72, lambda i, o: w.sweep_device(i, len(sweeps), o, T | BRUTE)) == host["sweeps"].tobytes()
        res["sweeps_plain"] = records(sweeps, 72, lambda i, o: w.sweep_device(i, len(sweeps), o, 0)) == host["sweeps_plain"].tobytes()
        for name, flags, want in (("overlaps", T, host["overlaps"]), ("overlaps_brute", T | BRUTE, host["overlaps"]), ("overlaps_plain", 0, host["overlaps_plain"])):
            offsets, raw = overlaps(flags, len(want[1]))
            res[name] = bool(np.array_equal(offsets, want[0])) and raw == want[1].tobytes()
        offsets, _ = overlaps(T, 0)
        res["overlaps_count_only"] = bool(np.array_equal(offsets, host["overlaps"][0]))
        # without the flag the device variants of the world WITH a terrain (above) answered as the host variants; so do those of
        # the same world after set_terrain(NULL)
        w.set_terrain(None)
        res["rays_plain_no_terrain"] = records(rays, 64, lambda i, o: w.raycast_device(i, len(rays), o, 0)) == host["rays_plain"].tobytes()
        res["rays_masked_no_terrain"] = records(rays, 64, lambda i, o: w.raycast_device(i, len(rays), o, 0, mask=2)) == w.raycast(rays, mask=2).tobytes()
        res["sweeps_plain_no_terrain"] = records(sweeps, 72, lambda i, o: w.sweep_device(i, len(sweeps), o, 0)) == host["sweeps_plain"].tobytes()
        offsets, raw = overlaps(0, len(host["overlaps_plain"][1]))
        res["overlaps_plain_no_terrain"] = bool(np.array_equal(offsets, host["overlaps_plain"][0])) and raw == host["overlaps_plain"][1].tobytes()
        res["guard"] = guard
    w.set_stream(0)
    w.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
