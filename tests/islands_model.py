"""Independent model of the contact islands (include/xpbd.h, "Contact ISLANDS") in plain Python / numpy.

Takes what a host can download -- the bodies, the frame's pair records, the joints, the last substep's contact masks -- and
the call's flags, groups the non-fixed bodies by breadth-first search (the library uses a union-find) and builds the records
exactly as the header defines them.  Every output is an integer or a bit pattern, so the comparison with the library is exact."""
from collections import deque

import numpy as np

ISLAND_NONE = 0xFFFFFFFF
NO_JOINTS, NO_CONTACTS = 1, 2
ISLAND_DTYPE = np.dtype([("first_body", "<u4"), ("n_bodies", "<u4"), ("n_pairs", "<u4"), ("n_joints", "<u4"), ("n_anchors", "<u4"),
                         ("n_grounded", "<u4"), ("max_speed2", "<f8"), ("max_angular_speed2", "<f8")])
SIGN_CLEARED = np.uint64(0x7FFFFFFFFFFFFFFF)


def fixed_bodies(bodies):
    """inverse_mass == 0 and all nine inverse_inertia entries == 0 (columns 0 and 1..9 of an xpbd_rigid)."""
    b = np.asarray(bodies, dtype=np.float64).reshape(-1, 38)
    return np.all(b[:, 0:10] == 0.0, axis=1)


def speed2_bits(v):
    """v.x * v.x + v.y * v.y + v.z * v.z, left to right, as the bit pattern with the sign cleared."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        s = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    return np.ascontiguousarray(s).view(np.uint64) & SIGN_CLEARED


def masks_from_contacts(n, contacts):
    """Per-body masks of the last substep from the (body, vertex) list of xpbd_world_download_contacts."""
    masks = np.zeros(n, dtype=np.uint32)
    c = np.asarray(contacts, dtype=np.uint32).reshape(-1, 2)
    np.bitwise_or.at(masks, c[:, 0], np.uint32(1) << (c[:, 1] & 31))
    return masks


def _ends(edges, a="body_a", b="body_b"):
    """[(a, b)] of pair records, joint records or an (m, 2) array."""
    if edges is None or len(edges) == 0:
        return []
    e = np.asarray(edges)
    if e.dtype.names:
        return [(int(x), int(y)) for x, y in zip(e[a], e[b])]
    return [(int(x), int(y)) for x, y in e.reshape(-1, 2)]


def islands(bodies, pairs, joints, masks, flags=0):
    """(island_of [n] uint32, ISLAND_DTYPE records) of the world as downloaded."""
    b = np.asarray(bodies, dtype=np.float64).reshape(-1, 38)
    n = b.shape[0]
    fixed = fixed_bodies(b)
    contact_edges = [] if flags & NO_CONTACTS else _ends(pairs)
    joint_edges = [] if flags & NO_JOINTS else _ends(joints)
    adjacent = [[] for _ in range(n)]
    for x, y in contact_edges + joint_edges:
        if not fixed[x] and not fixed[y]:
            adjacent[x].append(y)
            adjacent[y].append(x)
    island_of = np.full(n, ISLAND_NONE, dtype=np.uint32)
    members = []
    for start in range(n):                      # ascending: an island is first met at its smallest member
        if fixed[start] or island_of[start] != ISLAND_NONE:
            continue
        k = len(members)
        island_of[start] = k
        group, queue = [], deque([start])
        while queue:
            x = queue.popleft()
            group.append(x)
            for y in adjacent[x]:
                if island_of[y] == ISLAND_NONE:
                    island_of[y] = k
                    queue.append(y)
        members.append(sorted(group))
    out = np.zeros(len(members), dtype=ISLAND_DTYPE)
    v2, a2 = speed2_bits(b[:, 22:25]), speed2_bits(b[:, 25:28])
    grounded = np.asarray(masks).reshape(-1) != 0
    for k, group in enumerate(members):
        out["first_body"][k] = group[0]
        out["n_bodies"][k] = len(group)
        out["n_grounded"][k] = int(np.count_nonzero(grounded[group]))
        out["max_speed2"][k] = np.array([v2[group].max()], dtype=np.uint64).view(np.float64)[0]
        out["max_angular_speed2"][k] = np.array([a2[group].max()], dtype=np.uint64).view(np.float64)[0]
    for field, edges in (("n_pairs", contact_edges), ("n_joints", joint_edges)):
        for x, y in edges:
            if fixed[x] and fixed[y]:
                continue
            if fixed[x] or fixed[y]:
                out["n_anchors"][island_of[y if fixed[x] else x]] += 1
            else:
                assert island_of[x] == island_of[y]
                out[field][island_of[x]] += 1
    return island_of, out


def same_bytes(a, b):
    """Bit-for-bit equality of two arrays (record arrays included: doubles compare as bits, a NaN equals the same NaN)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
