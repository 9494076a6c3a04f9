"""Shared by test_gpu_sleeping.py and its torch child process (sleep_device_child.py): the scenes, what one frame leaves behind
for the comparisons, and the frame-by-frame comparison of a world's sleep state with the independent model (sleep_model.py)."""
import numpy as np

import islands_common as ic
import islands_model as im
import sleep_model as sm
from constraint_solver_amd import capi

DT = ic.DT
SUBSTEPS = 20
GAP = 0.002
CFG = (0.1, 0.5, 30)                  # linear_speed, angular_speed, frames_to_sleep of the stack scenes
LOOSE = (0.5, 2.0, 5)                 # ... of the box drop: many groups sleep and wake
STACK, SINGLE, FALLING, DROPPER = (0, 1, 2), 3, 4, 5


def stack_scene(dropper=False):
    """Bodies 0-2: a 3-stack of unit boxes with a 2 mm gap; 3: a single box on the plane 20 m away; 4: a box in free fall from
    z = 50, 40 m away; with `dropper` 5: a box 5 m above the stack's top."""
    n = 6 if dropper else 5
    bodies, _ = capi.scene_generate(ic.BOXES, 3, n)
    bodies[:, 22:28] = 0.0
    bodies[:, 34:38] = [1.0, 0.0, 0.0, 0.0]
    at = np.zeros((n, 3))
    for k in STACK:
        at[k] = [0.0, 0.0, k * (1.0 + GAP)]
    at[SINGLE] = [20.0, 0.0, 0.0]
    at[FALLING] = [40.0, 0.0, 50.0]
    if dropper:
        at[DROPPER] = [0.0, 0.0, 3 * (1.0 + GAP) + 5.0]
    bodies[:, 31:34] = at
    return bodies, np.zeros(n, dtype=np.uint32)


def stack_world(dropper=False, sleeping=CFG, trace=False):
    bodies, sid = stack_scene(dropper)
    w = capi.World(mode=capi.MODE_CONTACTS, trace_contacts=trace)
    w.set_polytopes(capi.scene_polytopes(ic.BOXES))
    w.upload(bodies, sid)
    w.set_contact_report(True)
    if sleeping:
        w.set_sleeping(*sleeping)
    return w, ic.distance_joints([], [])


def crafted_world(sleeping=CFG):
    w, joints = ic.crafted_world()
    if sleeping:
        w.set_sleeping(*sleeping)
    return w, joints


def drop_world(narrowphase=capi.NARROWPHASE_SAT, sleeping=LOOSE):
    w, joints = ic.drop_world(narrowphase, fixed=(5, 200))
    if sleeping:
        w.set_sleeping(*sleeping)
    return w, joints


class Frame:
    """What a host can see after one step."""

    def __init__(self, w, state=True):
        self.bodies = w.download()
        self.pairs = w.pair_contacts(points=False)[0]
        self.events = w.contact_events()
        self.counts = w.contact_report_counts()
        self.contacts = np.asarray(w.contacts()).copy()
        if state:
            self.asleep, self.rest_frames, self.group, self.sleep_counts = w.sleep_state()


def assert_state_equals_model(f, model, woken, slept, where):
    assert im.same_bytes(f.asleep, model.asleep), (where, "asleep", np.flatnonzero(f.asleep != model.asleep)[:8])
    assert im.same_bytes(f.rest_frames, model.rest_frames), (where, "rest_frames", np.flatnonzero(f.rest_frames != model.rest_frames)[:8],
                                                             f.rest_frames[:8], model.rest_frames[:8])
    assert im.same_bytes(f.group, model.group), (where, "group", np.flatnonzero(f.group != model.group)[:8])
    assert f.sleep_counts == model.counts() + (woken, slept), (where, f.sleep_counts, model.counts(), woken, slept)


def run_against_model(w, joints, cfg, frames, substeps=SUBSTEPS, requests=None, state=None, first_frame=1):
    """Steps `frames` frames; after each the library's state must equal the model's.  requests: {frame: sleep_model.Requests} made
    (by the caller's hook in `requests[frame].apply`) before that frame.  Returns (the frames, the model's last state)."""
    state = state if state is not None else sm.State(w.n)
    out = []
    for k in range(first_frame, first_frame + frames):
        req = (requests or {}).get(k)
        if req is not None and getattr(req, "apply", None):
            req.apply(w)
        w.step(DT, substeps)
        f = Frame(w)
        state, woken, slept = sm.frame(state, f.bodies, f.pairs, joints, cfg, req)
        assert_state_equals_model(f, state, woken, slept, "frame %d" % k)
        out.append(f)
    return out, state


def run_with_twin(make, frames, cfg=CFG, substeps=SUBSTEPS):
    """make(sleeping: bool) -> (world, joints).  The world with sleeping on, held to the model after every frame, and its twin that
    never sleeps: (frames of the first, frames of the twin)."""
    w, joints = make(True)
    with w:
        slept, _ = run_against_model(w, joints, cfg, frames, substeps=substeps)
    t, _ = make(False)
    with t:
        twin = []
        for _ in range(frames):
            t.step(DT, substeps)
            twin.append(Frame(t, state=False))
    return slept, twin


DYN = list(range(22, 28)) + list(range(31, 38))          # the 13 dynamic doubles of an xpbd_rigid row


def contacts_of(frame, body):
    c = frame.contacts.reshape(-1, 2)
    return c[c[:, 0] == body].tobytes()


def assert_frozen(frames):
    """Rule (a) and (b) over a run in which nobody made a request: no report pair has two inert ends; a body asleep during a frame
    keeps its 13 doubles and its ground contacts bit for bit, its velocities +0.0.  Returns how many (body, frame) it checked."""
    fixed = im.fixed_bodies(frames[0].bodies)
    checked = 0
    for k in range(1, len(frames)):
        prev, cur = frames[k - 1], frames[k]
        during = prev.asleep.astype(bool)                    # asleep during frame k = after the pass of k - 1
        inert = during | fixed
        for p in cur.pairs:
            assert not (inert[p["body_a"]] and inert[p["body_b"]]), (k + 1, int(p["body_a"]), int(p["body_b"]))
        for i in np.flatnonzero(during):
            assert im.same_bytes(prev.bodies[i, DYN], cur.bodies[i, DYN]), (k + 1, i)
            assert np.all(cur.bodies[i, 22:28].view(np.uint64) == 0), (k + 1, i)         # +0.0
            assert contacts_of(prev, i) == contacts_of(cur, i), (k + 1, i)
            checked += 1
    return checked


def assert_twin(frames, twin, far=()):
    """Until the first island sleeps everything is the twin's bits; after that the bodies `far` from every sleeper are, for as
    long as they have been awake since the start.  Returns how many (far body, frame) it compared."""
    first = next(k for k, f in enumerate(frames) if f.sleep_counts[3])
    assert first > 0
    for k in range(first):
        assert im.same_bytes(frames[k].bodies, twin[k].bodies), k + 1
        assert frames[k].counts == twin[k].counts and im.same_bytes(frames[k].events, twin[k].events), k + 1
    compared = 0
    for i in far:
        for k in range(len(frames)):
            if frames[k].asleep[i]:
                break
            assert im.same_bytes(frames[k].bodies[i], twin[k].bodies[i]), (i, k + 1)
            compared += 1
    return compared
