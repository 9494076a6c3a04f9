"""Shared by test_gpu_body_edits.py and its torch child process (body_edit_device_child.py): the 130-body scenes, the edit
lists and the A/B runs."""
import numpy as np

from constraint_solver_amd import capi
from halo_common import pile

DT = 1.0 / 60.0
N = 130                      # more than two waves, no multiple of 64, and the SoA stride (256) differs from it
FRAMES, SUBSTEPS = 3, 20
STATIC_BODY = 100


def scene(kind, seed=7):
    """The small pile of the other contact tests (mixed: the three shapes of tests/golden/mixed48.json; or boxes), body
    STATIC_BODY immovable."""
    bodies, sid = pile(capi, kind, N, seed, 5.0, 6.0)
    bodies[STATIC_BODY, 0:10] = 0.0
    bodies[STATIC_BODY, 22:28] = 0.0                                     # ... and at rest, above the ground
    bodies[STATIC_BODY, 33] = 3.0
    return bodies, sid


def world(kind, bodies, sid, mode=capi.MODE_CONTACTS, narrowphase=capi.NARROWPHASE_SAT):
    w = capi.World(mode=mode)
    w.set_polytopes(capi.scene_polytopes(kind))
    if mode == capi.MODE_CONTACTS:
        w.set_narrowphase(narrowphase)
    w.upload(bodies, sid)
    return w


def stepped(w, frames=FRAMES, substeps=SUBSTEPS):
    """(bodies, contacts) after `frames` frames."""
    for _ in range(frames):
        w.step(DT, substeps)
    return w.download(), w.contacts()


def wrench_values(seed, n=N):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 30.0, (n, 3)), rng.normal(0.0, 4.0, (n, 3))


def impulse_list(bodies, seed):
    """300 entries, SORTED by body: single entries on bodies 0..62, a run on body 63 at list positions 63..66 (across the
    first wave boundary), a run of 70 on body 64 (longer than a wave), three entries on each of the bodies 65..113 (the
    static one among them), single entries on the rest; both flags; impulses of about 1 m/s times the body's mass."""
    rng = np.random.default_rng(seed)
    counts = np.ones(N, dtype=np.int64)
    counts[63], counts[64] = 4, 70
    counts[65:114] += 2
    body = np.repeat(np.arange(N, dtype=np.uint32), counts)
    assert body.size == 300 and np.flatnonzero(body == 63).tolist() == [63, 64, 65, 66] and counts[STATIC_BODY] == 3
    mass = np.where(bodies[body, 0] > 0.0, 1.0 / np.where(bodies[body, 0] > 0.0, bodies[body, 0], 1.0), 1.0)
    out = np.zeros(body.size, dtype=capi.IMPULSE_DTYPE)
    out["body"] = body
    out["flags"] = rng.integers(0, 2, body.size)
    out["impulse"] = rng.normal(0.0, 1.0, (body.size, 3)) * mass[:, None]
    out["point"] = bodies[body, 31:34] + bodies[body, 28:31] + rng.uniform(-0.5, 0.5, (body.size, 3))
    out["angular_impulse"] = rng.normal(0.0, 0.05, (body.size, 3)) * mass[:, None]
    out["point"][out["flags"] == capi.IMPULSE_AT_CENTRE] = np.nan      # ignored with AT_CENTRE, by every variant
    return out


def shuffled(entries, seed):
    return entries[np.random.default_rng(seed).permutation(entries.size)]


def presorted(entries):
    """What the host variant makes of a list: sorted by body, the entries of a body in their list order."""
    return entries[np.argsort(entries["body"], kind="stable")]
