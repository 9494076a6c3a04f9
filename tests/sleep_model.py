"""Independent model of island sleeping (include/xpbd.h, "SLEEPING") in plain Python / numpy, on top of islands_model.py.

Takes what a host can download after a frame -- the bodies, the report's touching pairs, the joints -- with the state before
the frame and the wake requests made since the frame before, and returns the state after the frame's sleep pass.  Every
output is an integer, so the comparison with the library is exact.

The velocities the pass judges are those the last substep left.  The download shows +0.0 for a body the pass has just put to
sleep; a body only goes to sleep in a frame in which it was at rest, and +0.0 is at rest under every configuration, so the
downloaded bodies give the same counters."""
import numpy as np

import islands_model as im

GROUP_NONE = 0xFFFFFFFF
U32_MAX = 0xFFFFFFFF


class State:
    def __init__(self, n):
        self.asleep = np.zeros(n, dtype=np.uint8)
        self.rest_frames = np.zeros(n, dtype=np.uint32)
        self.group = np.full(n, GROUP_NONE, dtype=np.uint32)

    def copy(self):
        s = State(len(self.asleep))
        s.asleep, s.rest_frames, s.group = self.asleep.copy(), self.rest_frames.copy(), self.group.copy()
        return s

    def counts(self):
        """(asleep bodies, sleeping groups)"""
        idx = np.flatnonzero(self.asleep)
        return len(idx), len(set(int(g) for g in self.group[idx]))


class Requests:
    """Wake requests between two frames: bodies named by an edit or a wake call, wake-everybody, zero-all-counters."""

    def __init__(self, bodies=(), wake_all=False, zero_counters=False):
        self.bodies, self.wake_all, self.zero_counters = list(bodies), wake_all, zero_counters


def _wake(state, who):
    state.asleep[who] = 0
    state.rest_frames[who] = 0
    state.group[who] = GROUP_NONE


def _wake_groups(state, marked_bodies):
    """Every sleeper whose group is the group of a marked sleeper wakes; returns how many."""
    groups = {int(state.group[s]) for s in marked_bodies if state.asleep[s]}
    who = [i for i in range(len(state.asleep)) if state.asleep[i] and int(state.group[i]) in groups]
    _wake(state, who)
    return len(who)


def frame_begin(state, fixed, requests):
    """The state the frame runs with: the requests applied, before the broadphase."""
    s = state.copy()
    req = requests or Requests()
    wake_all = req.wake_all or any(fixed[i] for i in req.bodies)
    if wake_all:
        _wake(s, np.flatnonzero(s.asleep))
    else:
        _wake_groups(s, req.bodies)
    if req.zero_counters:
        s.rest_frames[:] = 0
    return s


def at_rest(bodies, linear_speed, angular_speed):
    b = np.asarray(bodies, dtype=np.float64).reshape(-1, 38)
    with np.errstate(all="ignore"):
        v, w = b[:, 22:25], b[:, 25:28]
        v2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
        w2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
        return (v2 <= linear_speed * linear_speed) & (w2 <= angular_speed * angular_speed)   # a NaN compares false


def sleep_pass(state, bodies, pairs, joints, linear_speed, angular_speed, frames_to_sleep):
    """(state after the pass, bodies woken, bodies put to sleep) from the state the frame ran with."""
    b = np.asarray(bodies, dtype=np.float64).reshape(-1, 38)
    n = b.shape[0]
    fixed = im.fixed_bodies(b)
    s = state.copy()
    # 1. wake
    marked = []
    for x, y in im._ends(pairs):
        for sleeper, other in ((x, y), (y, x)):
            if s.asleep[sleeper] and not s.asleep[other] and not fixed[other]:
                marked.append(sleeper)
    woken = _wake_groups(s, marked)
    # 2. count
    rest = at_rest(b, linear_speed, angular_speed)
    for i in range(n):
        if s.asleep[i] or fixed[i]:
            continue
        s.rest_frames[i] = min(int(s.rest_frames[i]) + 1, U32_MAX) if rest[i] else 0
    # 3. sleep
    island_of, records = im.islands(b, pairs, joints, np.zeros(n, dtype=np.uint32), 0)
    slept = 0
    for k in range(len(records)):
        members = np.flatnonzero(island_of == k)
        if np.any(s.asleep[members]) or np.any(s.rest_frames[members] < frames_to_sleep):
            continue
        s.asleep[members] = 1
        s.group[members] = records["first_body"][k]
        slept += len(members)
    return s, woken, slept


def frame(state, bodies, pairs, joints, cfg, requests=None):
    """One xpbd_world_step: (state after it, woken, slept).  cfg = (linear_speed, angular_speed, frames_to_sleep)."""
    fixed = im.fixed_bodies(bodies)
    return sleep_pass(frame_begin(state, fixed, requests), bodies, pairs, joints, *cfg)
