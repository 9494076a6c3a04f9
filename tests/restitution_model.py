"""Independent model of one substep of the contact pipeline WITH restitution (include/xpbd.h, "RESTITUTION"), in plain Python
floats, built on material_model.py: stages 1 to 5 are that model's (broadphase, integrate and SAT from the oracle; ground
contacts, Jacobi pair pass and derive restated there), stage 6 -- the velocity pass after derive -- is written here, operation
by operation in the header's order.  With every coefficient 0 no contact makes an entry, so the model must equal the oracle bit
for bit (tests/test_restitution_model.py proves that first).

Scenes are joint-free, SAT only, as material_model.py."""
import ctypes as C

import numpy as np

import material_model as mm
import oracle_binding as ob
from material_model import add, cross, divs, dot, frame_mulv, lscale, magnitude, mat3_mulv, qrot, scale, sub

UP = (0.0, 0.0, 1.0)


class VelBody:
    """What stage 6 reads of a body: pose and velocities after derive, velocities at the start of the substep, mass properties."""

    def __init__(self, row, vel0, ang0):
        b = mm.Body(row)
        self.inv_mass, self.inv_inertia, self.com, self.pos, self.rot = b.inv_mass, b.inv_inertia, b.com, b.pos, b.rot
        self.vel = tuple(float(x) for x in row[22:25])
        self.ang = tuple(float(x) for x in row[25:28])
        self.vel0, self.ang0 = vel0, ang0


def larger(a, b):
    return b if a < b else a


def bounces(e, threshold, vn0, w):
    """Whether a contact takes part in stage 6: it closed faster than the threshold when the substep started."""
    return e > 0.0 and vn0 < -threshold and w > 0.0


SWEEPS = 4          # XPBD_RESTITUTION_SWEEPS: passes over the points of one manifold (include/xpbd.h: XPBD_RESTITUTION_SWEEPS)


def manifold_entry(self_is_inc, inc, ref, points, e, threshold):
    """(dv, dw) of one manifold for the incident or the reference body, and the number of impulses applied: SWEEPS sequential
    passes over `points` ((p_inc, p_ref, n) each) on copies of the two bodies' post-derive velocities."""
    v_inc, w_inc, v_ref, w_ref = inc.vel, inc.ang, ref.vel, ref.ang
    c_inc, c_ref = add(inc.pos, inc.com), add(ref.pos, ref.com)
    applied = 0
    total = [0.0] * len(points)                      # the impulse every point has applied so far: never negative
    for _ in range(SWEEPS):
        for k, (p_inc, p_ref, n) in enumerate(points):
            arm_inc, arm_ref = sub(p_inc, c_inc), sub(p_ref, c_ref)
            u_inc, u_ref = add(v_inc, cross(w_inc, arm_inc)), add(v_ref, cross(w_ref, arm_ref))
            u0_inc, u0_ref = add(inc.vel0, cross(inc.ang0, arm_inc)), add(ref.vel0, cross(ref.ang0, arm_ref))
            vn, vn0 = dot(n, sub(u_inc, u_ref)), dot(n, sub(u0_inc, u0_ref))
            w = mm.inverse_resistance(inc, p_inc, n) + mm.inverse_resistance(ref, p_ref, n)
            if not bounces(e, threshold, vn0, w):
                continue
            wanted = total[k] + (-e * vn0 - vn) / w
            if not wanted > 0.0:
                wanted = 0.0
            lam = wanted - total[k]
            if lam == 0.0:
                continue
            total[k] = wanted
            plus, minus = lscale(lam, n), lscale(-lam, n)
            v_inc, w_inc = add(v_inc, scale(plus, inc.inv_mass)), add(w_inc, cross(mat3_mulv(inc.inv_inertia, arm_inc), plus))
            v_ref, w_ref = add(v_ref, scale(minus, ref.inv_mass)), add(w_ref, cross(mat3_mulv(ref.inv_inertia, arm_ref), minus))
            applied += 1
    if self_is_inc:
        return sub(v_inc, inc.vel), sub(w_inc, inc.ang), applied
    return sub(v_ref, ref.vel), sub(w_ref, ref.ang), applied


def ground_bounce(body, vertices, mask, e, threshold):
    """The ground part of stage 6 on `body` (velocities updated in place); returns the number of entries."""
    entries = 0
    if not (e > 0.0 and mask):
        return entries
    origin = add(add(body.pos, body.com), qrot(body.rot, mm.neg(body.com)))          # Rigid::frame() at the pose after derive
    centre = add(body.pos, body.com)
    for v, vertex in enumerate(vertices):
        if not mask >> v & 1:
            continue
        p = frame_mulv((origin, body.rot), vertex)
        arm = sub(p, centre)
        vn = dot(UP, add(body.vel, cross(body.ang, arm)))
        vn0 = dot(UP, add(body.vel0, cross(body.ang0, arm)))
        w = mm.inverse_resistance(body, p, UP)
        target = -e * vn0
        if not (bounces(e, threshold, vn0, w) and vn < target):
            continue
        lam = (target - vn) / w
        impulse = lscale(lam, UP)
        body.vel = add(body.vel, scale(impulse, body.inv_mass))
        body.ang = add(body.ang, cross(mat3_mulv(body.inv_inertia, arm), impulse))
        entries += 1
    return entries


class Model(mm.Model):
    """material_model.Model plus restitution `e[n]`, `ground_e` and `bounce_threshold`.  pair_entries (manifolds that bounced, counted from both of their bodies),
    pair_impulses (impulses inside them, counted once) and ground_entries count what stage 6 did, summed over the substeps run."""

    def __init__(self, bodies, sid, polys, e=None, ground_e=0.0, bounce_threshold=0.0, **materials):
        super().__init__(bodies, sid, polys, **materials)
        self.e = [0.0] * self.n if e is None else [float(x) for x in e]
        self.ground_e = float(ground_e)
        self.threshold = float(bounce_threshold)
        self.pair_entries = self.pair_impulses = self.ground_entries = 0

    def substep(self, off, nb, h):
        L = ob.load()
        n, rows = self.n, self.bodies
        start = [(tuple(float(x) for x in rows[i, 22:25]), tuple(float(x) for x in rows[i, 25:28])) for i in range(n)]
        # what stage 6 needs of stages 1 and 2, which the base class keeps to itself: the post-integrate frames (the oracle's
        # integrate on a copy), from them the ground masks and, for the face contacts, the reference planes
        p1, masks = [], []
        for i in range(n):
            r = ob.Rigid.from_np(rows[i])
            L.o_rigid_integrate(C.byref(r), h)
            f = L.o_rigid_frame(C.byref(r))
            p1.append(f)
            frame = mm._frame_of(f)
            mask = 0
            for v, vertex in enumerate(self.verts[int(self.sid[i])]):
                if not frame_mulv(frame, vertex)[2] >= 0.0:
                    mask |= 1 << v
            masks.append(mask)
        super().substep(off, nb, h)                                   # stages 1 to 5
        if not (self.ground_e > 0.0 or any(x > 0.0 for x in self.e)):
            return
        state = [VelBody(rows[i], *start[i]) for i in range(n)]
        manifolds = {}
        out = []
        for b in range(n):
            dv, dw, count = (0.0, 0.0, 0.0), (0.0, 0.0, 0.0), 0
            for j in nb[off[b]:off[b + 1]]:
                j = int(j)
                lo, hi = (b, j) if b < j else (j, b)
                if (lo, hi) not in manifolds:
                    manifolds[(lo, hi)] = self.manifold(p1, lo, hi)
                m = manifolds[(lo, hi)]
                if m is None:
                    continue
                feature, normal, p_ref, p_inc = m
                ref, inc = (lo, hi) if feature != ob.FEATURE_FACE_B else (hi, lo)
                e = larger(self.e[inc], self.e[ref])
                if not e > 0.0:
                    continue
                points = []
                for pt in range(len(p_ref)):
                    if normal is not None:
                        nrm = normal
                    else:
                        d = sub(p_ref[pt], p_inc[pt])
                        length = magnitude(d)
                        if length == 0.0:
                            continue
                        nrm = scale(d, 1.0 / length)
                    points.append((p_inc[pt], p_ref[pt], nrm))
                tv, tw, applied = manifold_entry(inc == b, state[inc], state[ref], points, e, self.threshold)
                if applied:
                    dv, dw, count = add(dv, tv), add(dw, tw), count + 1
                    if inc == b:
                        self.pair_impulses += applied
            out.append((dv, dw, count))
            self.pair_entries += count
        for b in range(n):
            dv, dw, count = out[b]
            body = VelBody(rows[b], *start[b])
            if count:
                cnt = float(count)
                body.vel, body.ang = add(body.vel, divs(dv, cnt)), add(body.ang, divs(dw, cnt))
            self.ground_entries += ground_bounce(body, self.verts[int(self.sid[b])], masks[b], larger(self.e[b], self.ground_e), self.threshold)
            rows[b, 22:25], rows[b, 25:28] = body.vel, body.ang

    def manifold(self, p1, i, j):
        """(feature, reference plane normal or None, p_ref[], p_inc[]) of pair i < j at the post-integrate frames, or None:
        the same pre-test and SAT call as material_model.Model.substep."""
        L = ob.load()
        si, sj = int(self.sid[i]), int(self.sid[j])
        fi, fj = mm._frame_of(p1[i]), mm._frame_of(p1[j])
        between = sub(frame_mulv(fj, self.centroid[sj]), frame_mulv(fi, self.centroid[si]))
        reach = self.radius[si] + self.radius[sj]
        if not dot(between, between) < reach * reach:
            return None
        raw = [(f.position.np(), f.rotation.np()) for f in (p1[i], p1[j])]
        m = ob.sat(raw[0], raw[1], self.polys[si], self.polys[sj])
        if m.separated or not m.n_points:
            return None
        ref, inc = m.points()
        normal = None
        if m.feature != ob.FEATURE_EDGES:
            body, shape, face = (i, si, m.index_a) if m.feature == ob.FEATURE_FACE_A else (j, sj, m.index_b)
            plane = L.o_frame_mulplane(p1[body], L.o_polytope_plane(C.byref(self.polys[shape]), face))
            normal = tuple(float(x) for x in plane.normal.np())
        return int(m.feature), normal, [tuple(float(x) for x in p) for p in ref], [tuple(float(x) for x in p) for p in inc]


# ---- scenes and bounds of the physics tests (CPU model and GPU alike) ------------------------------------------------------
# Every figure below was MEASURED on this model (20 substeps, dt = 1/60) before its bound was chosen; DESIGN.md 8, "Restitution".
G = 9.81
DROP_HEIGHT = 2.0
# A box dropped flat from 2 m: upward speed at the end of the bounce frame over the downward speed at the end of the frame
# before it, minus e.  Measured -0.046 (e = 0.5) and -0.052 (e = 0.8): the frame in which the box lands also holds up to 1/60 s
# of gravity on either side of the bounce (g dt (1 + e) / 6.2 m/s = up to 0.04), and the four corners bounce one after the
# other, which leaves the box turning at 2.5 to 3.1 rad/s.  Bound: 0.08, 1.5 times the worse measurement.
DROP_RATIO_BOUND = 0.08
# Rebound apex over e^2 H, minus 1: measured -0.127 (e = 0.5) and -0.098 (e = 0.8), the square of the above.  Bound: 0.2.
DROP_APEX_BOUND = 0.2
# Two equal boxes head-on at +-1 m/s, face to face (a four-point manifold), no forces: relative speed after over before, minus
# e.  Measured +5.2e-5 for e = 1 (velocities exchanged; what is left is the convergence of four sweeps: 7.6e-3 with two,
# 8.6e-10 with eight) and +0.0611 for e = 0.5: the substep of the bounce ends at 0.50004, and the position pass of the NEXT
# substep pushes the remaining overlap out, which derive turns into 0.061 m/s more (with e = 1 the boxes have separated by
# then).  Bounds: 1e-3 and 0.1.  Sideways and angular velocity afterwards: at most 1.7e-4 (m/s, rad/s), bound 1e-3.  Momentum:
# 2e-13 m/s, bound 1e-10.
HEAD_ON_BOUND = {1.0: 1e-3, 0.5: 0.1}
HEAD_ON_SPIN_BOUND = 1e-3
HEAD_ON_MOMENTUM_BOUND = 1e-10


def bounce_frame(vz):
    """Index of the first frame that ends with the box moving up, in a list of vertical velocities per frame."""
    return next(k for k, v in enumerate(vz) if v > 0.0)


def apex_after(z, k):
    """Largest height from frame k on until the box comes down again."""
    while k + 1 < len(z) and z[k + 1] >= z[k]:
        k += 1
    return z[k]


def dropped_box(capi, height, g=G):
    """One unit cube (local [0, 1]^3, density 1), axis-aligned, at rest with its bottom face `height` above the ground."""
    bodies, sid, _ = mm.resting_box(capi, 0.0, z=height, g=g)
    return bodies, sid


def head_on_boxes(capi, speed, gap=0.5, z=5.0):
    """Two equal unit cubes far above the ground, no forces, approaching each other along x with +-speed, faces parallel."""
    bodies, sid = capi.scene_generate(capi.SCENE_BOXES, 1, 2)
    for k, b in enumerate(bodies):
        b[34:38] = [1.0, 0.0, 0.0, 0.0]
        b[10:28] = 0.0
        b[31:34] = [k * (1.0 + gap), 0.0, z]
        b[22] = speed if k == 0 else -speed
    return bodies, sid
