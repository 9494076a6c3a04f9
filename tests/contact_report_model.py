"""Model of the contact REPORTS (include/xpbd.h, "Contact REPORTS") on top of the CPU oracle: which neighbour pairs touch at
the post-integrate poses P1 of a substep (oracle/xpbd_pairs_oracle.h, steps 1-2), the pair records and points of the last
substep, and the begin / end events between two frames' touching sets."""
import ctypes as C
import math

import numpy as np

import oracle_binding as ob
from constraint_solver_amd import capi


def p1_frames(bodies, h):
    """Rigid::frame() of every body after Rigid::integrate(h): (position[3], rotation[4]) tuples."""
    L = ob.load()
    out = []
    for b in bodies:
        r = ob.Rigid.from_np(b)
        L.o_rigid_integrate(C.byref(r), h)
        f = L.o_rigid_frame(C.byref(r))
        out.append((f.position.np(), f.rotation.np()))
    return out


def upper_pairs(offsets, neighbours):
    """The pair list (i, j), i < j, of CSR neighbour lists, sorted."""
    out = []
    for i in range(len(offsets) - 1):
        for j in neighbours[offsets[i]:offsets[i + 1]]:
            if j > i:
                out.append((i, int(j)))
    return out


def manifolds(frames, sid, polys, pairs):
    """{(i, j): oracle Manifold} of the pairs that touch (op_sat: not separated, n_points > 0)."""
    out = {}
    for i, j in pairs:
        m = ob.sat(frames[i], frames[j], polys[int(sid[i])], polys[int(sid[j])])
        if not m.separated and m.n_points > 0:
            out[(i, j)] = m
    return out


def _norm(u):
    return math.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2])


def record(frames, sid, polys, i, j, m):
    """(feature, n_points, normal[3], depth, p_ref (k, 3), p_inc (k, 3)) of a touching pair's manifold, as the report gives it."""
    L = ob.load()
    ref, inc = m.points()
    feature = int(m.feature)
    if feature == capi.FEATURE_EDGES:
        u = [float(ref[0][a]) - float(inc[0][a]) for a in range(3)]
        g = _norm(u)
        normal = [u[a] * (1.0 / g) for a in range(3)] if g != 0.0 else [0.0, 0.0, 0.0]
    else:
        body, face = (i, m.index_a) if feature == capi.FEATURE_FACE_A else (j, m.index_b)
        pos, rot = frames[body]
        plane = L.o_frame_mulplane(ob.frame(pos, rot), L.o_polytope_plane(C.byref(polys[int(sid[body])]), int(face)))
        normal = list(plane.normal.np())
        if feature == capi.FEATURE_FACE_B:
            normal = [-v for v in normal]
    depth = 0.0
    for k in range(int(m.n_points)):
        g = _norm([float(ref[k][a]) - float(inc[k][a]) for a in range(3)])
        depth = g if g > depth else depth
    return feature, int(m.n_points), np.array(normal), depth, ref, inc


def events(prev, cur):
    """(body_a, body_b, kind) of the documented event order: BEGINs (cur - prev), then ENDs (prev - cur), each sorted."""
    prev, cur = set(prev), set(cur)
    return [(a, b, capi.CONTACT_BEGIN) for a, b in sorted(cur - prev)] + [(a, b, capi.CONTACT_END) for a, b in sorted(prev - cur)]
