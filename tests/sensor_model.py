"""Sensor occupancy (include/xpbd.h, "SENSOR bodies") as pure Python, from what a host can download: the report's pair records
(sorted by (body_a, body_b), every record a pair that touched in the frame) and the sensor table.  occupancy() is written the way
the header words it -- per sensor, the bodies that touched it, ascending, with the index of the pair's record; brute_force()
restates it body by body without the sorted order.  No device, no library."""
import numpy as np

HIT_DTYPE = np.dtype([("body", "<u4"), ("pair", "<u4")])


def occupancy(body_a, body_b, is_sensor):
    """(sensors, offsets, hits): sensors ascending; hits[offsets[k]:offsets[k + 1]] the other ends of the records with sensors[k]
    at one end, ascending by body, `pair` = the record's index."""
    body_a, body_b = np.asarray(body_a, dtype=np.int64), np.asarray(body_b, dtype=np.int64)
    sensors = np.flatnonzero(np.asarray(is_sensor)).astype(np.uint32)
    offsets, hits = [0], []
    for s in sensors:
        mine = [(int(body_b[r]), r) for r in np.flatnonzero(body_a == s)] + [(int(body_a[r]), r) for r in np.flatnonzero(body_b == s)]
        hits += sorted(mine)
        offsets.append(len(hits))
    out = np.zeros(len(hits), dtype=HIT_DTYPE)
    if hits:
        out["body"], out["pair"] = zip(*hits)
    return sensors, np.array(offsets, dtype=np.uint32), out


def brute_force(body_a, body_b, is_sensor):
    """The same lists as [(sensor, [(body, record), ...]), ...], found by asking for every (sensor, body) whether a record names
    the two."""
    where = {(int(a), int(b)): r for r, (a, b) in enumerate(zip(body_a, body_b))}
    out = []
    for s in range(len(is_sensor)):
        if not is_sensor[s]:
            continue
        found = []
        for j in range(len(is_sensor)):
            r = where.get((min(s, j), max(s, j))) if j != s else None
            if r is not None:
                found.append((j, r))
        out.append((s, found))
    return out


def as_lists(sensors, offsets, hits):
    """(sensors, offsets, hits) in brute_force's form."""
    return [(int(s), [(int(h["body"]), int(h["pair"])) for h in hits[offsets[k]:offsets[k + 1]]]) for k, s in enumerate(sensors)]
