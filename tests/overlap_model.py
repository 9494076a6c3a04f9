"""Independent model of the overlap queries (include/xpbd.h, "Overlap queries"): every query against every body on the CPU.

Per (query, body) pair, in the order of the definition: ignore_body and the group mask; the tight bounding spheres, with
centres from the oracle's o_frame_mulv and the comparison in plain Python floats (between = centre_b - centre_q, reach =
radius_q + radius_b, dot(between, between) < reach * reach); the oracle's op_sat for the survivors, of which only the verdict
(separated == 0), the feature and the separation are kept.  Body frames are the oracle's o_rigid_frame of the downloaded
bodies.  Nothing here shares code with the library.

Polytopes are dicts as capi.World.set_polytopes takes them; bodies are (n, 38) xpbd_rigid rows; queries are
capi.OVERLAP_QUERY_DTYPE records."""
import ctypes as C
import math

import numpy as np

import oracle_binding as ob

NO_HIT = 0xFFFFFFFF
HIT_DTYPE = np.dtype([("body", "<u4"), ("feature", "<u4"), ("separation", "<f8")])


def oracle_polytope(poly):
    """The oracle's Polytope struct of a set_polytopes dict (same vertex, edge and face order)."""
    v = np.asarray(poly["vertices"], dtype=np.float64).reshape(-1, 3)
    e = np.asarray(poly["edges"]).reshape(-1, 2)
    fo, fi = np.asarray(poly["face_offsets"]), np.asarray(poly["face_indices"])
    p = ob.Polytope()
    p.n_vertices, p.n_edges, p.n_faces = len(v), len(e), len(fo) - 1
    assert p.n_vertices <= 32 and p.n_edges <= 64 and p.n_faces <= 32 and len(fi) <= 128
    for i, x in enumerate(v):
        p.vertices[i] = ob.vec3(x)
    for i, x in enumerate(e):
        p.edges[i][0], p.edges[i][1] = int(x[0]), int(x[1])
    for i, x in enumerate(fo):
        p.face_offsets[i] = int(x)
    for i, x in enumerate(fi):
        p.face_indices[i] = int(x)
    p.centroid = ob.vec3(poly["centroid"])
    return p


def shape_radius(poly):
    """max |vertex - centroid| as xpbd_world_set_polytopes computes it: sqrt((x * x + y * y) + z * z)."""
    c = [float(x) for x in poly["centroid"]]
    r = 0.0
    for v in np.asarray(poly["vertices"], dtype=np.float64).reshape(-1, 3):
        d = (float(v[0]) - c[0], float(v[1]) - c[1], float(v[2]) - c[2])
        r = max(r, math.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))
    return r


class Scene:
    """The bodies' side of the model, computed once and shared by the queries of a test."""

    def __init__(self, bodies, shape_id, polytopes, groups=None):
        L = ob.load()
        self.L = L
        self.polys = [oracle_polytope(p) for p in polytopes]
        self.radii = [shape_radius(p) for p in polytopes]
        self.centroids = [ob.vec3(p["centroid"]) for p in polytopes]
        self.sid = [int(s) for s in shape_id]
        b = np.asarray(bodies, dtype=np.float64).reshape(-1, 38)
        self.frames = [L.o_rigid_frame(C.byref(ob.Rigid.from_np(row))) for row in b]
        self.centres = np.array([L.o_frame_mulv(f, self.centroids[s]).np() for f, s in zip(self.frames, self.sid)]).reshape(-1, 3)
        self.body_radius = np.array([self.radii[s] for s in self.sid])
        self.groups = None if groups is None else [int(g) for g in groups]
        ident = (np.zeros(3), np.array([1.0, 0.0, 0.0, 0.0]))
        ob.sat(ident, ident, self.polys[0], self.polys[0])           # (declares op_sat's signature)

    def query(self, q, masked=False, census=None):
        """[(body, feature, separation)] of one query record, ascending in body.  census (a dict) counts the pairs whose
        spheres overlap ('spheres') and those of them the SAT separates ('sat_rejects')."""
        sq = int(q["shape"])
        if sq >= len(self.polys):
            return []
        fq = ob.frame(q["position"], q["rotation"])
        cq = self.L.o_frame_mulv(fq, self.centroids[sq])
        cq, rq = (cq.x, cq.y, cq.z), self.radii[sq]
        with np.errstate(all="ignore"):                               # a generous numpy pre-selection; the decision is below
            d = self.centres - np.array(cq)
            near = np.nonzero(~((d * d).sum(axis=1) >= ((rq + self.body_radius) * 1.001) ** 2))[0]
        out = []
        ignore, mask = int(q["ignore_body"]), int(q["mask"])
        for i in near:
            i = int(i)
            if i == ignore:
                continue
            if masked and ((0xFFFFFFFF if self.groups is None else self.groups[i]) & mask) == 0:
                continue
            cb = self.centres[i]
            between = (float(cb[0]) - cq[0], float(cb[1]) - cq[1], float(cb[2]) - cq[2])
            reach = rq + self.radii[self.sid[i]]
            if not (between[0] * between[0] + between[1] * between[1] + between[2] * between[2] < reach * reach):
                continue
            if census is not None:
                census["spheres"] = census.get("spheres", 0) + 1
            m = ob.Manifold()
            self.L.op_sat(fq, self.frames[i], C.byref(self.polys[sq]), C.byref(self.polys[self.sid[i]]), C.byref(m))
            if m.separated:
                if census is not None:
                    census["sat_rejects"] = census.get("sat_rejects", 0) + 1
                continue
            out.append((i, int(m.feature), float(m.separation)))
        return out

    def overlap(self, queries, masked=False, census=None):
        """(offsets, hits) as the library returns them."""
        offsets, hits = [0], []
        for q in np.asarray(queries).reshape(-1):
            hits += self.query(q, masked, census)
            offsets.append(len(hits))
        return np.array(offsets, dtype=np.uint32), np.array(hits, dtype=HIT_DTYPE).reshape(-1)


def overlap(bodies, shape_id, polytopes, queries, masked=False, groups=None, census=None):
    return Scene(bodies, shape_id, polytopes, groups).overlap(queries, masked, census)
