"""Independent model of the collision filters (include/xpbd.h, "Collision FILTERS"): which neighbour pairs of the sphere
broadphase survive a list of {group, mask} per body and, with XPBD_FILTER_JOINTED, a joint list.  Plain numpy, no device."""
import numpy as np

ALL = 0xFFFFFFFF


def may_touch(filters, i, j):
    """The pair rule: (group_i & mask_j) != 0 and (group_j & mask_i) != 0 (filters None: every pair may)."""
    if filters is None:
        return True
    gi, mi = int(filters["group"][i]), int(filters["mask"][i])
    gj, mj = int(filters["group"][j]), int(filters["mask"][j])
    return (gi & mj) != 0 and (gj & mi) != 0


def joined_pairs(joints):
    """{(min, max)} of the bodies every joint links."""
    if joints is None:
        return set()
    return {(min(int(a), int(b)), max(int(a), int(b))) for a, b in zip(joints["body_a"], joints["body_b"])}


def filter_lists(offsets, neighbours, filters=None, joints=None, jointed=False):
    """CSR neighbour lists (ascending per body) without the pairs the filters exclude; the order of what stays is kept."""
    joined = joined_pairs(joints) if jointed else set()
    out_off, out_nb = [0], []
    for i in range(len(offsets) - 1):
        for j in neighbours[offsets[i]:offsets[i + 1]]:
            j = int(j)
            if may_touch(filters, i, j) and (min(i, j), max(i, j)) not in joined:
                out_nb.append(j)
        out_off.append(len(out_nb))
    return np.array(out_off, dtype=np.uint32), np.array(out_nb, dtype=np.uint32)


def is_symmetric(offsets, neighbours):
    """Every j in i's list has i in its own list (what the CSR's pair index relies on)."""
    pairs = set()
    for i in range(len(offsets) - 1):
        for j in neighbours[offsets[i]:offsets[i + 1]]:
            pairs.add((i, int(j)))
    return all((j, i) in pairs for i, j in pairs)


def admitted(filters, n, mask):
    """Bodies a masked ray cast may hit: (group & mask) != 0 (filters None: every body is in group ~0)."""
    groups = np.full(n, ALL, dtype=np.uint64) if filters is None else filters["group"].astype(np.uint64)
    return (groups & np.uint64(mask)) != 0
