"""Child process of tests/test_gpu_distance.py: the device variant of the distance queries with torch tensors on a torch stream
handed to the world with set_stream.  torch is imported first, so that the library binds to the HIP runtime torch carries (as in
bench.py).  Prints one JSON line of verdicts."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
from constraint_solver_amd import capi  # noqa: E402
import test_gpu_overlap as ov  # noqa: E402
import test_gpu_distance as t  # noqa: E402

GUARD = 16


def main():
    torch.cuda.set_device(0)
    bodies, sid = ov.pile(2048)
    polys = capi.scene_polytopes(t.KIND)
    w = ov.stepped(bodies, sid, polys, 1, 10)
    q, _ = t.distance_families(np.random.default_rng(16), w.download(), sid, polys, 384)
    hits = w.distance(q)
    stream = torch.cuda.Stream()
    w.set_stream(stream.cuda_stream)
    res = {"hits": int(np.sum(hits["body"] != capi.NO_HIT)) > 100}

    def run(batch, flags):
        dev_q = torch.from_numpy(batch.view(np.uint8).copy()).to("cuda")
        dev_hits = torch.full(((len(batch) + GUARD) * 96,), 0xEE, dtype=torch.uint8, device="cuda")
        w.distance_device(dev_q.data_ptr(), len(batch), dev_hits.data_ptr(), flags)
        # (the copy below is ordered after the query on the same stream)
        return dev_hits.cpu().numpy()

    with torch.cuda.stream(stream):
        guard = True
        for name, batch, flags in (("grid", q, 0), ("brute", q, t.BRUTE), ("few", q[48:55], 0)):
            raw = run(batch, flags)
            res[name] = raw[:len(batch) * 96].tobytes() == hits[:len(batch)].tobytes() if name != "few" else raw[:7 * 96].tobytes() == hits[48:55].tobytes()
            guard = guard and bool((raw[len(batch) * 96:] == 0xEE).all())
        res["guard"] = guard
    w.set_stream(0)
    w.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
