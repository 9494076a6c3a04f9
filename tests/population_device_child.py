"""Child process of test_gpu_population.py: xpbd_world_remove_bodies_device driven from torch tensors on a torch stream handed
to the world with set_stream.  A process of its own that imports torch first, so that the library binds to the HIP runtime
torch carries (as bench.py and body_edit_device_child.py do).  Writes its arrays to the .npz named on the command line and
prints one JSON line; the parent compares them with the host variant."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]

from constraint_solver_amd import capi  # noqa: E402
import body_edit_common as bc  # noqa: E402
import population_common as pc  # noqa: E402

CAP = 64


def main(out_path):
    torch.cuda.set_device(0)
    kind = capi.SCENE_BOXES_DROP
    bodies, sid = bc.scene(kind)
    stream = torch.cuda.Stream()
    res, verdict = {}, {"cap": CAP}
    with torch.cuda.stream(stream):
        # flags a kernel of the stream has just written, the map into a tensor; the world carries every setting
        w = bc.world(kind, bodies, sid)
        w.set_stream(stream.cuda_stream)
        pc.apply_settings(w, pc.settings_for())
        w.step(bc.DT, bc.SUBSTEPS)
        listed = torch.from_numpy(pc.REMOVED.astype(np.int64)).to("cuda")
        flags = torch.zeros(bc.N, dtype=torch.uint8, device="cuda").index_fill_(0, listed, 3)      # any nonzero byte removes
        dev_map = torch.full((bc.N,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        res["flags_joint_map"] = w.remove_bodies_device(flags.data_ptr(), dev_map.data_ptr())
        res["flags_map"] = dev_map.cpu().numpy().view(np.uint32)
        res["flags_changed"] = w.download()
        w.step(bc.DT, bc.SUBSTEPS)
        res["flags_stepped"] = w.download()
        w.set_stream(0)
        w.close()

        # no flag set: nothing changes, the history stays
        w = bc.world(kind, bodies, sid)
        w.set_stream(stream.cuda_stream)
        w.history_push()
        none = torch.zeros(bc.N, dtype=torch.uint8, device="cuda")
        dev_map = torch.full((bc.N,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        w.remove_bodies_device(none.data_ptr(), dev_map.data_ptr())
        res["none_map"] = dev_map.cpu().numpy().view(np.uint32)
        res["none_history"] = np.int64(w.history_length())
        w.set_stream(0)
        w.close()

        # "who is inside this trigger?" -> gone, without a host round trip between the query and the removal
        w = bc.world(kind, bodies, sid)
        w.set_stream(stream.cuda_stream)
        w.step(bc.DT, bc.SUBSTEPS)
        q = pc.trigger_volume()
        dev_q = torch.from_numpy(q.view(np.uint8).copy()).to("cuda")
        dev_off = torch.zeros(len(q) + 1, dtype=torch.int32, device="cuda")
        dev_hits = torch.zeros(CAP * 4, dtype=torch.int32, device="cuda")        # xpbd_overlap_hit: body, feature, separation
        w.overlap_device(dev_q.data_ptr(), len(q), dev_off.data_ptr(), dev_hits.data_ptr(), CAP)
        valid = torch.arange(CAP, device="cuda") < dev_off[len(q)]
        body = torch.where(valid, dev_hits.view(CAP, 4)[:, 0], torch.full((CAP,), bc.N, dtype=torch.int32, device="cuda")).long()
        counts = torch.zeros(bc.N + 1, dtype=torch.int32, device="cuda").index_add_(0, body, torch.ones(CAP, dtype=torch.int32, device="cuda"))
        flags = (counts[:bc.N] > 0).to(torch.uint8)
        dev_map = torch.full((bc.N,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        w.remove_bodies_device(flags.data_ptr(), dev_map.data_ptr())
        verdict["hits"] = int(dev_off[len(q)].item())
        res["trigger_map"] = dev_map.cpu().numpy().view(np.uint32)
        res["trigger_changed"] = w.download()
        w.set_stream(0)
        w.close()
    np.savez(out_path, **res)
    print(json.dumps(verdict))


if __name__ == "__main__":
    main(sys.argv[1])
