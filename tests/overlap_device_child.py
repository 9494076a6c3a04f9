"""Child process of tests/test_gpu_overlap.py: the device variant of the overlap queries with torch tensors on a torch stream
handed to the world with set_stream.  torch is imported first, so that the library binds to the HIP runtime torch carries (as
in bench.py).  Prints one JSON line of verdicts."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from constraint_solver_amd import capi  # noqa: E402
import test_gpu_overlap as t  # noqa: E402

GUARD = 64


def main():
    torch.cuda.set_device(0)
    bodies, sid = t.pile(2048)
    polys = capi.scene_polytopes(t.KIND)
    w = t.stepped(bodies, sid, polys, 10)
    q = t.query_families(np.random.default_rng(6), w.download(), sid, polys, 384)
    offsets, hits = w.overlap(q)
    total = len(hits)
    stream = torch.cuda.Stream()
    w.set_stream(stream.cuda_stream)
    res = {"hits": total > 100}

    def run(cap, flags):
        dev_q = torch.from_numpy(q.view(np.uint8).copy()).to("cuda")
        dev_off = torch.full((len(q) + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        dev_hits = torch.full(((cap + GUARD) * 16,), 0xEE, dtype=torch.uint8, device="cuda")
        w.overlap_device(dev_q.data_ptr(), len(q), dev_off.data_ptr(), dev_hits.data_ptr(), cap, flags)
        # (the copies below are ordered after the query on the same stream)
        return dev_off.cpu().numpy().view(np.uint32), dev_hits.cpu().numpy()

    with torch.cuda.stream(stream):
        for name, flags in (("grid", 0), ("brute", t.BRUTE)):
            off, raw = run(total, flags)
            res[name] = t.same_bits(off, offsets) and raw[:total * 16].tobytes() == hits.tobytes() and bool((raw[total * 16:] == 0xEE).all())
        cap = int(offsets[np.argmax(np.diff(offsets.astype(np.int64)))]) + 1      # inside the longest segment
        off, raw = run(cap, 0)
        res["short_total"] = t.same_bits(off, offsets) and int(off[-1]) == total
        res["short_prefix"] = raw[:cap * 16].tobytes() == hits[:cap].tobytes()
        res["short_guard"] = bool((raw[cap * 16:] == 0xEE).all())
    w.set_stream(0)
    w.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
