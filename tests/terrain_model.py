"""Independent model of the contact pipeline on a heightfield TERRAIN (include/xpbd.h, "TERRAIN"), in plain Python floats,
built on material_model.py and restitution_model.py (imported, not edited): the lookup and the terrain forms of the ground
contacts (stage 3) and of restitution's ground part (stage 6) are restated here, operation by operation in the header's order;
the broadphase, integrate and the SAT come from the oracle and the pair pass, derive and the pair part of stage 6 from the two
models, as in material_model.Model.

Those two models call their ground stages as module-level functions (material_model.ground_contacts,
restitution_model.ground_bounce), so Model.substep puts the terrain forms in their place for the duration of one substep and
runs the inherited pipeline: nothing else of it is touched.  With a flat field under every body the model must equal
material_model.Model bit for bit (tests/test_terrain_model.py proves that first).

Scenes are joint-free, SAT only, as material_model.py."""
import math

import numpy as np

import material_model as mm
import restitution_model as rm
from material_model import add, cross, dot, frame_mulv, lscale, magnitude, mat3_mulv, scale, sub

NAN = math.nan
TWO52 = 4503599627370496.0          # from here on every double is an integer (or inf): floor is the identity


def _floor(u):
    return float(math.floor(u)) if u < TWO52 else u


class Terrain:
    """xpbd_heightfield: heights[iy][ix] at (origin[0] + ix * cell[0], origin[1] + iy * cell[1])."""

    def __init__(self, heights, origin, cell):
        h = np.asarray(heights, dtype=np.float64)
        assert h.ndim == 2 and h.shape[0] >= 2 and h.shape[1] >= 2
        self.ny, self.nx = h.shape
        self.H = [[float(x) for x in row] for row in h]
        self.x0, self.y0 = float(origin[0]), float(origin[1])
        self.dx, self.dy = float(cell[0]), float(cell[1])

    def plane(self, x):
        """(n, d) of the triangle over or under world point x, or None outside the field: steps 1 to 6 of the header."""
        u = (x[0] - self.x0) / self.dx
        v = (x[1] - self.y0) / self.dy
        if not (u >= 0.0 and v >= 0.0):
            return None
        fi, fj = _floor(u), _floor(v)
        if not (fi < self.nx - 1 and fj < self.ny - 1):
            return None
        i, j = int(fi), int(fj)
        fu, fv = u - fi, v - fj
        h00, h10, h01, h11 = self.H[j][i], self.H[j][i + 1], self.H[j + 1][i], self.H[j + 1][i + 1]
        if fu >= fv:
            sx, sy = (h10 - h00) / self.dx, (h11 - h10) / self.dy
        else:
            sx, sy = (h11 - h01) / self.dx, (h01 - h00) / self.dy
        raw = (-sx, -sy, 1.0)
        n = scale(raw, 1.0 / magnitude(raw))
        d = dot(n, (self.x0 + fi * self.dx, self.y0 + fj * self.dy, h00))
        return n, d

    def sample(self, x, y):
        """(height, normal) as xpbd_world_sample_terrain reports them."""
        p = self.plane((x, y, 0.0))
        if p is None:
            return NAN, (0.0, 0.0, 0.0)
        n, d = p
        return (d - (n[0] * x + n[1] * y)) / n[2], n


def signed_distance(plane, x):
    return dot(plane[0], x) - plane[1]


def ground_contacts(terrain, body, p1, past, vertices, mu, compliance, limit, trace=None):
    """material_model.ground_contacts with the terrain's plane under every vertex in place of z = 0.  Returns the mask."""
    constraints, mask = [], 0
    for v, vertex in enumerate(vertices):
        x = frame_mulv(p1, vertex)
        plane = terrain.plane(x)
        if plane is None:
            continue
        s = signed_distance(plane, x)
        if s >= 0.0:
            continue
        mask |= 1 << v
        n = plane[0]
        target = (x[0] - s * n[0], x[1] - s * n[1], x[2] - s * n[2])
        correction = sub(target, x)
        delta = mm.frame_delta(p1, past, x)
        delta_tangential = sub(delta, mm.project_on(delta, correction))
        k = mm.friction_factor(mu, correction, delta_tangential)
        constraints.append((x, sub(target, lscale(k, delta_tangential)), delta, correction))
    for c0, c1, delta, correction in constraints:
        difference = sub(c1, c0)
        distance = magnitude(difference)
        direction = scale(difference, mm._div(1.0, distance))
        w = mm.inverse_resistance(body, c0, direction)
        error = mm.allowed_error(distance, limit, delta, correction)
        lagrange = mm._div(error - 0.0, w + compliance)
        impulse = lscale(lagrange, direction)
        if trace is not None:
            trace.append((direction, impulse))
        body.pos = add(body.pos, scale(impulse, body.inv_mass))
        arm = sub(c0, add(body.pos, body.com))
        spin = (0.0, cross(mat3_mulv(body.inv_inertia, arm), impulse))
        body.rot = mm.qnormalize(mm.qadd(body.rot, mm.qmul(mm.qlscale(0.5, spin), body.rot)))
    return mask


def ground_bounce(terrain, body, vertices, mask, e, threshold):
    """restitution_model.ground_bounce with the lookup repeated at every vertex of the mask: outside the field no entry,
    inside the plane's normal in place of (0, 0, 1)."""
    entries = 0
    if not (e > 0.0 and mask):
        return entries
    origin = add(add(body.pos, body.com), mm.qrot(body.rot, mm.neg(body.com)))
    centre = add(body.pos, body.com)
    for v, vertex in enumerate(vertices):
        if not mask >> v & 1:
            continue
        p = frame_mulv((origin, body.rot), vertex)
        plane = terrain.plane(p)
        if plane is None:
            continue
        n = plane[0]
        arm = sub(p, centre)
        vn = dot(n, add(body.vel, cross(body.ang, arm)))
        vn0 = dot(n, add(body.vel0, cross(body.ang0, arm)))
        w = mm.inverse_resistance(body, p, n)
        target = -e * vn0
        if not (rm.bounces(e, threshold, vn0, w) and vn < target):
            continue
        lam = (target - vn) / w
        impulse = lscale(lam, n)
        body.vel = add(body.vel, scale(impulse, body.inv_mass))
        body.ang = add(body.ang, cross(mat3_mulv(body.inv_inertia, arm), impulse))
        entries += 1
    return entries


class Model(rm.Model):
    """restitution_model.Model (material_model.Model when no coefficient of restitution is set) standing on `terrain`
    (a Terrain, or None for the plane z = 0).  masks: the ground contact masks of the last substep run."""

    def __init__(self, bodies, sid, polys, terrain=None, **settings):
        super().__init__(bodies, sid, polys, **settings)
        self.terrain = terrain
        self.masks = [0] * self.n

    def substep(self, off, nb, h):
        if self.terrain is None:
            return super().substep(off, nb, h)
        terrain, masks, bounced = self.terrain, [], []

        def contacts(body, p1, past, vertices, mu, compliance, limit, trace=None):      # called for body 0, 1, ... in turn
            masks.append(ground_contacts(terrain, body, p1, past, vertices, mu, compliance, limit, trace))

        def bounce(body, vertices, _plane_mask, e, threshold):                            # likewise; the mask is stage 3's
            bounced.append(None)
            return ground_bounce(terrain, body, vertices, masks[len(bounced) - 1], e, threshold)

        plain = mm.ground_contacts, rm.ground_bounce
        mm.ground_contacts, rm.ground_bounce = contacts, bounce
        try:
            super().substep(off, nb, h)
        finally:
            mm.ground_contacts, rm.ground_bounce = plain
        assert len(masks) == self.n and len(bounced) in (0, self.n)
        self.masks = masks


# ---- fields and scenes of the tests (CPU model and GPU alike) ---------------------------------------------------------------
def flat_field(nx, ny):
    return np.zeros((ny, nx))


def tilted_field(nx, ny, origin, cell, slope_x, slope_y=0.0):
    """heights of the plane h = slope_x * x + slope_y * y at the samples."""
    x = origin[0] + np.arange(nx) * cell[0]
    y = origin[1] + np.arange(ny) * cell[1]
    return slope_x * x[None, :] + slope_y * y[:, None]


def bumpy_field(nx, ny, seed, amplitude=0.5):
    return np.random.default_rng(seed).uniform(-amplitude, amplitude, (ny, nx))


def box_on_slope(capi, tan_theta, at=(0.0, 0.0), g=9.81):
    """(bodies, shape ids, theta, downhill): one unit cube (local [0, 1]^3, density 1) at rest under plain gravity -z with its
    bottom face lying ON the plane h = tan_theta * x: corner (0, 0, 0) of the cube at the plane's point over `at`, the cube
    turned by -theta about y.  downhill: the unit vector along the slope, pointing down."""
    bodies, sid, _ = mm.resting_box(capi, 0.0, g=g)
    b = bodies[0]
    theta = math.atan(tan_theta)
    half = -0.5 * theta
    rot = (math.cos(half), (0.0, math.sin(half), 0.0))
    com = tuple(float(x) for x in b[28:31])
    corner = (at[0], at[1], tan_theta * at[0])
    pos = add(sub(corner, com), mm.qrot(rot, com))             # Rigid::frame().position = pos + com - rot * com = corner
    b[31:34] = pos
    b[34], b[35:38] = rot[0], rot[1]
    return bodies, sid, theta, (-math.cos(theta), 0.0, -math.sin(theta))
