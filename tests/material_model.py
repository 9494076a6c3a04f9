"""Independent model of one substep of the contact pipeline WITH contact materials (include/xpbd.h, "Contact MATERIALS"), in
plain Python floats: IEEE f64, one rounding per operation, nothing contracted.

From the CPU oracle (tests/oracle_binding.py) it takes only what friction does not touch: the broadphase, Rigid::integrate
and Rigid::frame (steps 1 of oracle/xpbd_pairs_oracle.h), and the SAT of step 2.  Steps 3 to 5 -- the ground contacts, the
Jacobi pass over the pair contact points with the depenetration limit, and derive -- are restated here with the friction
factor k in place of the reference's literal 1.0, operation by operation in the oracle's order, so that with every
coefficient +inf the model must equal the oracle bit for bit (tests/test_material_model.py proves that first).

Scenes are joint-free: the model has no joints (friction does not touch them, and the oracle covers them)."""
import ctypes as C
import math

import numpy as np

import oracle_binding as ob

INF = math.inf


# ---- cgmath, as oracle/xpbd_oracle.c restates it: tuples of Python floats ---------------------------------------------------
def add(a, b):
    return (a[0] + b[0], a[1] + b[1], a[2] + b[2])


def sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def neg(a):
    return (-a[0], -a[1], -a[2])


def scale(a, s):            # Vector * scalar
    return (a[0] * s, a[1] * s, a[2] * s)


def lscale(s, a):           # scalar * Vector
    return (s * a[0], s * a[1], s * a[2])


def divs(a, s):
    return (a[0] / s, a[1] / s, a[2] / s)


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def cross(a, b):
    return ((a[1] * b[2]) - (a[2] * b[1]), (a[2] * b[0]) - (a[0] * b[2]), (a[0] * b[1]) - (a[1] * b[0]))


def magnitude(a):
    return math.sqrt(dot(a, a))


def project_on(a, onto):
    return scale(onto, _div(dot(a, onto), dot(onto, onto)))


def _div(a, b):
    """IEEE division: Python raises on a zero divisor where C gives inf / NaN."""
    if b == 0.0:
        if a == 0.0 or a != a:
            return math.nan
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


# quaternions: (s, (x, y, z))
def qmul(a, b):
    (s, v), (t, w) = a, b
    return (s * t - v[0] * w[0] - v[1] * w[1] - v[2] * w[2],
            (s * w[0] + v[0] * t + v[1] * w[2] - v[2] * w[1],
             s * w[1] + v[1] * t + v[2] * w[0] - v[0] * w[2],
             s * w[2] + v[2] * t + v[0] * w[1] - v[1] * w[0]))


def qrot(q, rhs):
    s, v = q
    tmp = add(cross(v, rhs), scale(rhs, s))
    return add(scale(cross(v, tmp), 2.0), rhs)


def qconj(q):
    return (q[0], neg(q[1]))


def qadd(a, b):
    return (a[0] + b[0], add(a[1], b[1]))


def qlscale(s, q):
    return (s * q[0], lscale(s, q[1]))


def qnormalize(q):
    k = _div(1.0, math.sqrt(q[0] * q[0] + dot(q[1], q[1])))
    return (q[0] * k, scale(q[1], k))


def mat3_mulv(m, v):        # m: three columns
    return add(add(scale(m[0], v[0]), scale(m[1], v[1])), scale(m[2], v[2]))


# frames: (position, rotation)
def frame_inverse(f):
    inv = qconj(f[1])
    return (qrot(inv, neg(f[0])), inv)


def frame_mulv(f, v):
    return add(qrot(f[1], v), f[0])


def frame_delta(f, past, point):
    local = frame_mulv(frame_inverse(f), point)
    return sub(point, frame_mulv(past, local))


# ---- bodies -------------------------------------------------------------------------------------------------------------
class Body:
    """The fields of an xpbd_rigid row (38 doubles) that steps 3 to 5 read or write."""

    def __init__(self, row):
        r = [float(x) for x in row]
        self.inv_mass = r[0]
        self.inv_inertia = (tuple(r[1:4]), tuple(r[4:7]), tuple(r[7:10]))
        self.com = tuple(r[28:31])
        self.pos = tuple(r[31:34])
        self.rot = (r[34], tuple(r[35:38]))


def _frame_of(f):
    return (tuple(float(x) for x in f.position.np()), (float(f.rotation.s), tuple(float(x) for x in f.rotation.v.np())))


def friction_factor(mu, correction, delta_tangential):
    """k of include/xpbd.h: how much of the tangential slip the contact takes back.  1.0 is the reference's contact."""
    bound = mu * magnitude(correction)
    len_t = magnitude(delta_tangential)
    return bound / len_t if bound < len_t else 1.0


def inverse_resistance(body, point, direction):
    angular = qrot(qconj(body.rot), cross(sub(point, add(body.pos, body.com)), direction))
    return body.inv_mass + dot(mat3_mulv(body.inv_inertia, angular), angular)


def allowed_error(distance, limit, delta, correction):
    """The depenetration limit (op_contacts_set_max_depenetration_speed): uses delta and correction, not c1."""
    if not limit > 0.0:
        return distance
    length = magnitude(correction)
    closing = dot(delta, correction) / length if length > 0.0 else 0.0
    allowed = limit - closing
    if not allowed > 0.0:
        allowed = 0.0
    return allowed if distance > allowed else distance


# ---- step 3: ground contacts, sequential per body -----------------------------------------------------------------------
def ground_contacts(body, p1, past, vertices, mu, compliance, limit, trace=None):
    """collision::ground on the frozen post-integrate frame p1, then solver::solve over its constraints in push order."""
    constraints = []
    for v in vertices:
        x = frame_mulv(p1, v)
        if x[2] >= 0.0:
            continue
        target = (x[0], x[1], 0.0)
        correction = sub(target, x)
        delta = frame_delta(p1, past, x)
        delta_tangential = sub(delta, project_on(delta, correction))
        k = friction_factor(mu, correction, delta_tangential)
        constraints.append((x, sub(target, lscale(k, delta_tangential)), delta, correction))
    for c0, c1, delta, correction in constraints:
        difference = sub(c1, c0)
        distance = magnitude(difference)
        direction = scale(difference, _div(1.0, distance))
        w = inverse_resistance(body, c0, direction)
        error = allowed_error(distance, limit, delta, correction)
        lagrange = _div(error - 0.0, w + compliance)
        impulse = lscale(lagrange, direction)
        if trace is not None:
            trace.append((direction, impulse))
        body.pos = add(body.pos, scale(impulse, body.inv_mass))
        arm = sub(c0, add(body.pos, body.com))
        spin = (0.0, cross(mat3_mulv(body.inv_inertia, arm), impulse))
        body.rot = qnormalize(qadd(body.rot, qmul(qlscale(0.5, spin), body.rot)))


# ---- step 4: one manifold point seen from one of its two bodies -----------------------------------------------------------
def pair_point(self_is_inc, inc, ref, inc_p1, inc_past, ref_p1, ref_past, p_inc, p_ref, mu, compliance, limit):
    correction = sub(p_ref, p_inc)
    delta_rel = sub(frame_delta(inc_p1, inc_past, p_inc), frame_delta(ref_p1, ref_past, p_ref))
    delta_tangential = sub(delta_rel, project_on(delta_rel, correction))
    k = friction_factor(mu, correction, delta_tangential)
    c0 = p_inc
    c1 = sub(p_ref, lscale(k, delta_tangential))
    difference = sub(c1, c0)
    distance = magnitude(difference)
    direction = scale(difference, _div(1.0, distance))
    w = inverse_resistance(inc, c0, direction) + inverse_resistance(ref, p_ref, direction)
    error = allowed_error(distance, limit, delta_rel, correction)
    lagrange = _div(error - 0.0, w + compliance)
    me = inc if self_is_inc else ref
    point = c0 if self_is_inc else p_ref
    impulse = lscale(lagrange, direction) if self_is_inc else lscale(-lagrange, direction)
    dpos = scale(impulse, me.inv_mass)
    arm = sub(point, add(me.pos, me.com))
    spin = (0.0, cross(mat3_mulv(me.inv_inertia, arm), impulse))
    return dpos, qmul(qlscale(0.5, spin), me.rot)


def shape_radius(poly):
    c = tuple(float(x) for x in poly.centroid.np())
    r = 0.0
    for v in poly.verts():
        d = magnitude(sub(tuple(float(x) for x in v), c))
        if d > r:
            r = d
    return r


# What the slope tests call sticking and sliding, as fractions of the distance g sin(theta) t^2 / 2 that a frictionless box
# covers.  The cases are far from the threshold on purpose (tan(theta) is half or twice mu): Coulomb leaves a sliding box
# 1 - mu / tan(theta) = 50 % of it, and a sticking one none.  The reference's own contact (mu = +inf) is compliant and creeps:
# measured on this model 0.1 % of the distance on the ground (1 s) and 1.5 % on a static slab body (0.5 s, tan(theta) = 0.25
# and 0.5).  STICKS is three times that, SLIDES is half of Coulomb's share.
STICKS, SLIDES = 0.05, 0.25


def resting_box(capi, tan_theta, z=0.0, g=9.81):
    """(bodies, shape ids, theta): one unit cube (local [0, 1]^3, density 1) at rest with its bottom face at height z, under
    gravity tilted by theta about y -- a slope of angle theta seen from the slope: the force on a body of mass m is
    m g (sin theta, 0, -cos theta), through external_force, since the ground stays z = 0."""
    bodies, sid = capi.scene_generate(capi.SCENE_BOXES, 1, 1)
    b = bodies[0]
    b[34:38] = [1.0, 0.0, 0.0, 0.0]
    b[22:28] = 0.0
    b[31:34] = [0.0, 0.0, z]
    theta = math.atan(tan_theta)
    mass = 1.0 / b[0]
    b[10:13] = [mass * g * math.sin(theta), 0.0, -mass * g * math.cos(theta)]
    b[13:22] = 0.0
    return bodies, sid, theta


def box_on_slab(capi, tan_theta, g=9.81):
    """(bodies, shape ids, theta, polytopes): resting_box on top of a STATIC slab body (a cube of edge 4 with inverse mass and
    inverse inertia 0, shape 1) instead of the ground: body 0 is the box, body 1 the slab; the box starts 1.5 m from the
    slab's edges."""
    box, _, theta = resting_box(capi, tan_theta, z=4.0, g=g)
    box[0, 31:33] = [1.5, 1.5]
    slab = capi.rigid_new(capi.rigid_metrics(capi.SHAPE_CUBE, 4.0, 1.0))
    slab[0:22] = 0.0                                            # immovable, no forces
    slab[22:28] = 0.0
    slab[31:34] = 0.0
    slab[34:38] = [1.0, 0.0, 0.0, 0.0]
    polys = [capi.polytope(capi.SHAPE_CUBE), capi.polytope(capi.SHAPE_CUBE, 4.0)]
    return np.stack([box[0], slab]), np.array([0, 1], dtype=np.uint32), theta, polys


class Model:
    """A joint-free world of `bodies` ((n, 38) rows) with shapes `polys` (oracle Polytope array), friction `mu[n]` and
    `ground_mu`; step(dt, substeps) is one frame of op_contacts_step with materials."""

    def __init__(self, bodies, sid, polys, mu=None, ground_mu=INF, pad=0.02, max_depenetration_speed=0.0):
        self.bodies = np.array(bodies, dtype=np.float64).reshape(-1, 38).copy()
        self.n = self.bodies.shape[0]
        self.sid = np.ascontiguousarray(sid if sid is not None else np.zeros(self.n), dtype=np.uint32)
        self.polys = polys
        self.mu = [INF] * self.n if mu is None else [float(m) for m in mu]
        self.ground_mu = float(ground_mu)
        self.pad = pad
        self.speed = max_depenetration_speed
        shapes = sorted(set(int(s) for s in self.sid))
        self.verts = {s: [tuple(float(x) for x in v) for v in polys[s].verts()] for s in shapes}
        self.centroid = {s: tuple(float(x) for x in polys[s].centroid.np()) for s in shapes}
        self.radius = {s: shape_radius(polys[s]) for s in shapes}
        self.ground_trace = None      # a list: step() appends (body, direction, impulse) of every ground constraint

    def step(self, dt, substeps):
        off, nb = ob.broadphase(self.bodies, self.sid, self.polys, dt, self.pad)
        h = dt / substeps
        for _ in range(substeps):
            self.substep(off, nb, h)
        return self.bodies

    def substep(self, off, nb, h):
        L = ob.load()
        n, rows = self.n, self.bodies
        compliance = 1e-6 / (h * h)
        limit = self.speed * h if self.speed > 0.0 else 0.0
        # 1. integrate (the oracle's), remembering the frames
        past, p1, past_pos, raw_p1 = [], [], [], []
        for i in range(n):
            r = ob.Rigid.from_np(rows[i])
            past.append(_frame_of(L.o_rigid_frame(C.byref(r))))
            past_pos.append(tuple(float(x) for x in rows[i, 31:34]))
            L.o_rigid_integrate(C.byref(r), h)
            f = L.o_rigid_frame(C.byref(r))
            raw_p1.append((f.position.np(), f.rotation.np()))
            p1.append(_frame_of(f))
            rows[i] = r.np()
        # 2. narrowphase on the post-integrate frames (the oracle's SAT behind its tight-sphere pre-test)
        manifolds = {}
        for i in range(n):
            for j in nb[off[i]:off[i + 1]]:
                j = int(j)
                if j <= i:
                    continue
                si, sj = int(self.sid[i]), int(self.sid[j])
                between = sub(frame_mulv(p1[j], self.centroid[sj]), frame_mulv(p1[i], self.centroid[si]))
                reach = self.radius[si] + self.radius[sj]
                if not dot(between, between) < reach * reach:
                    continue
                m = ob.sat(raw_p1[i], raw_p1[j], self.polys[si], self.polys[sj])
                if not m.separated and m.n_points:
                    ref, inc = m.points()
                    manifolds[(i, j)] = (int(m.feature), [tuple(float(x) for x in p) for p in ref], [tuple(float(x) for x in p) for p in inc])
        # 3. ground contacts
        state = [Body(rows[i]) for i in range(n)]
        for i in range(n):
            trace = [] if self.ground_trace is not None else None
            mu = min(self.mu[i], self.ground_mu)
            ground_contacts(state[i], p1[i], past[i], self.verts[int(self.sid[i])], mu, compliance, limit, trace)
            if trace:
                self.ground_trace.extend((i, d, p) for d, p in trace)
        # 4. pair contacts, Jacobi with averaging: reads state[], writes nxt[]
        nxt = []
        for b in range(n):
            dpos, drot, count = (0.0, 0.0, 0.0), (0.0, (0.0, 0.0, 0.0)), 0
            for j in nb[off[b]:off[b + 1]]:
                j = int(j)
                a_body, b_body = (b, j) if b < j else (j, b)
                m = manifolds.get((a_body, b_body))
                if m is None:
                    continue
                feature, p_ref, p_inc = m
                ref, inc = (a_body, b_body) if feature != ob.FEATURE_FACE_B else (b_body, a_body)
                mu = min(self.mu[inc], self.mu[ref])
                for pt in range(len(p_ref)):
                    tp, tr = pair_point(inc == b, state[inc], state[ref], p1[inc], past[inc], p1[ref], past[ref], p_inc[pt], p_ref[pt],
                                        mu, compliance, limit)
                    dpos, drot, count = add(dpos, tp), qadd(drot, tr), count + 1
            pos, rot = state[b].pos, state[b].rot
            if count:
                cnt = float(count)
                pos = add(pos, divs(dpos, cnt))
                rot = qnormalize(qadd(rot, (drot[0] / cnt, divs(drot[1], cnt))))
            nxt.append((pos, rot))
        # 5. derive
        for i in range(n):
            pos, rot = nxt[i]
            rows[i, 31:34] = pos
            rows[i, 34], rows[i, 35:38] = rot[0], rot[1]
            rows[i, 22:25] = divs(sub(pos, past_pos[i]), h)
            delta = qmul(rot, qconj(past[i][1]))
            if delta[0] < 0.0:
                delta = (-delta[0], neg(delta[1]))
            rows[i, 25:28] = divs(lscale(2.0, delta[1]), h)
