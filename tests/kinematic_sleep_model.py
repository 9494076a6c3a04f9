"""Independent model of island sleeping in a world with kinematic bodies (include/xpbd.h, "SLEEPING": the paragraph on MOVING
bodies), on top of sleep_model.py, whose pass it restates with one more source of marks.

A kinematic body is MOVING in a frame when the overwrite before its first substep gave it a nonzero velocity component
(kinematic_model.overwrite tells, from the bodies as they stood when the frame began).  In that frame it is not inert, so the
broadphase pairs it with sleepers; and wake step 1 also marks every sleeper that shares a pair of the frame's PAIR LIST (the
neighbour lists, not the touching set) or a joint with a MOVING body.  Everything else -- requests, counting, islands, who goes
to sleep -- is sleep_model's.  Every output is an integer, so the comparison with the library is exact."""
import numpy as np

import islands_model as im
import sleep_model as sm


def pair_list(offsets, neighbours):
    """The pairs (a < b) of a CSR neighbour list."""
    out = []
    for a in range(len(offsets) - 1):
        for b in neighbours[offsets[a]:offsets[a + 1]]:
            if a < int(b):
                out.append((a, int(b)))
    return out


def sleep_pass(state, bodies, pairs, joints, moving, frame_pairs, linear_speed, angular_speed, frames_to_sleep):
    """sleep_model.sleep_pass with the marks of the MOVING bodies: (state after the pass, bodies woken, bodies put to sleep)."""
    b = np.asarray(bodies, dtype=np.float64).reshape(-1, 38)
    n = b.shape[0]
    fixed = im.fixed_bodies(b)
    s = state.copy()
    # 1. wake: the touching set as before, then the pair list and the joints against the MOVING bodies
    marked = []
    for x, y in im._ends(pairs):
        for sleeper, other in ((x, y), (y, x)):
            if s.asleep[sleeper] and not s.asleep[other] and not fixed[other]:
                marked.append(sleeper)
    shared = list(frame_pairs) + [(int(j["body_a"]), int(j["body_b"])) for j in joints]
    for x, y in shared:
        for sleeper, other in ((x, y), (y, x)):
            if s.asleep[sleeper] and moving[other] and not moving[sleeper]:
                marked.append(sleeper)
    woken = sm._wake_groups(s, marked)
    # 2. count
    rest = sm.at_rest(b, linear_speed, angular_speed)
    for i in range(n):
        if s.asleep[i] or fixed[i]:
            continue
        s.rest_frames[i] = min(int(s.rest_frames[i]) + 1, sm.U32_MAX) if rest[i] else 0
    # 3. sleep: a kinematic body is a fixed body to the islands, an anchor and never a member
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


def frame(state, bodies, pairs, joints, cfg, moving, frame_pairs, requests=None):
    """One xpbd_world_step: (state after it, woken, slept).  moving[n]: who was MOVING in the frame; frame_pairs: its pair list."""
    fixed = im.fixed_bodies(bodies)
    return sleep_pass(sm.frame_begin(state, fixed, requests), bodies, pairs, joints, moving, frame_pairs, *cfg)


def may_pair(state_during, bodies, moving):
    """inert[n] of the frame: asleep, or fixed and not MOVING (no pair of the frame has two inert ends)."""
    return state_during.asleep.astype(bool) | (im.fixed_bodies(bodies) & ~np.asarray(moving, dtype=bool))
