"""Rigid bodies the scene generators never produce: non-zero internal force and torques, asymmetric and non-diagonal
inverse inertia, extreme and zero inverse mass, centres of mass away from the shape, far positions, fast spin, random hulls,
statics shared per shape but for one ulp, and heights exactly at the edges of the ground test.

`generate` is seeded and deterministic and returns (bodies (n, 38), shape_id, verts, offsets, labels).  Bodies stand on a
6 m grid so that no two bounding spheres overlap (the contacts pipeline then adds nothing to the ground path), and start
near or slightly inside the ground so that every category makes ground contacts.
"""
import numpy as np

from hull_util import random_hull

G = 9.81
PITCH = 6.0
CATEGORIES = ("plain", "force", "asym_inertia", "spd_inertia", "static_linear", "mass_extreme", "com_offset", "far", "spin",
              "hull", "ulp_shared")
# shape ids: the reference's three shapes as the scenes use them, two random hulls placed away from their centroid (one
# with topology for the contacts pipeline, one of XPBD_MAX_SHAPE_VERTS vertices, vertices only), and a copy of the cube
# that only the ulp_shared bodies use
CUBE, TETRA, ICOSA, HULL16, HULL32, ULP_CUBE = range(6)
N_SHAPES = 6


def _icosahedron(scale):
    phi = (1.0 + np.sqrt(5.0)) / 2.0
    mag = np.sqrt(phi * phi + 1.0)
    a, b = phi / mag, 1.0 / mag
    v = [(a, b, 0), (a, -b, 0), (-a, b, 0), (-a, -b, 0), (0, a, b), (0, a, -b), (0, -a, b), (0, -a, -b),
         (b, 0, a), (-b, 0, a), (b, 0, -a), (-b, 0, -a)]
    return scale * np.array(v, dtype=np.float64)


def _cube():
    return np.array([[(i & 1) * 1.0, (i >> 1 & 1) * 1.0, (i >> 2 & 1) * 1.0] for i in range(8)])


def _tetra(scale):
    return scale * np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])


def _hull16():
    pts, edges, faces, centroid = random_hull(2024, 16, 0.6)
    off = np.array([0.9, -0.7, 0.4])
    return pts + off, edges, faces, centroid + off


def _hull32():
    rng = np.random.default_rng(2025)
    p = rng.normal(size=(32, 3))
    p *= 0.7 / np.linalg.norm(p, axis=1, keepdims=True)          # on a sphere: every point is a vertex of the hull
    return p + np.array([-1.1, 0.6, 0.8])


def shapes():
    """Vertex tables of the six shapes, their centroids, and their topology (None for the vertex-only hull)."""
    cube, tet, ico = _cube(), _tetra(0.5), _icosahedron(0.5)
    h16, e16, f16, c16 = _hull16()
    h32 = _hull32()
    verts = [cube, tet, ico, h16, h32, cube]
    centroids = [np.full(3, 0.5), np.full(3, 0.125), np.zeros(3), c16, h32.mean(axis=0), np.full(3, 0.5)]
    return verts, centroids, {HULL16: (e16, f16)}


def polytopes():
    """capi.World.set_polytopes dicts of the six shapes in shape-id order.  HULL32 has no topology (more faces than a
    polytope may have): its slot holds the cube, and the contacts pipeline must not be given HULL32 bodies."""
    from constraint_solver_amd import capi
    from hull_util import as_capi
    verts, centroids, topo = shapes()
    cube = capi.polytope(capi.SHAPE_CUBE)
    h16 = as_capi(verts[HULL16], topo[HULL16][0], topo[HULL16][1], centroids[HULL16])
    return [cube, capi.polytope(capi.SHAPE_TETRAHEDRON, 0.5), capi.polytope(capi.SHAPE_ICOSAHEDRON, 0.5), h16, cube, cube]


def _random_rotation(rng):
    q = rng.uniform(-1.0, 1.0, 4)
    return q / np.sqrt(q[0] * q[0] + q[1:] @ q[1:])


def _rotate(q, v):
    u, s = q[1:], q[0]
    return v + 2.0 * np.cross(u, np.cross(u, v) + s * v)


def _asymmetric(rng, scale):
    """A random matrix far from symmetric: an antisymmetric part as large as its symmetric part, which is positive
    definite so that a constraint's inverse resistance m^-1 + (M a).a stays positive, as it does for a real body."""
    k = rng.normal(size=(3, 3))
    k = (k - k.T) / np.linalg.norm(k - k.T)
    s = _spd(rng, scale)
    return s + k * np.linalg.norm(s) * rng.uniform(0.7, 1.2)


def _spd(rng, scale):
    q = _random_rotation(rng)
    r = np.stack([_rotate(q, e) for e in np.eye(3)], axis=1)
    return r @ np.diag(rng.uniform(0.5, 2.0, 3) * scale) @ r.T


def set_matrix(body, m):
    """inverse_inertia[3*col + row] = m[row, col] (cgmath column-major)."""
    body[1:10] = np.asarray(m).T.reshape(9)


def generate(seed, per_category=8, h=1.0 / 1200.0):
    """Edge bodies for a step of substep length h (the spin category's angular speeds are scaled to it)."""
    rng = np.random.default_rng(seed)
    verts, centroids, _ = shapes()
    rows, sids, labels = [], [], []
    k = 0
    for cat in CATEGORIES:
        for j in range(per_category):
            b = np.zeros(38)
            sid = [CUBE, TETRA, ICOSA][j % 3]
            if cat == "hull":
                sid = (HULL16, HULL32)[j % 2]
            if cat == "ulp_shared":
                sid = ULP_CUBE
            im = rng.uniform(0.5, 2.0)
            m = np.diag(rng.uniform(2.0, 12.0, 3)) * im
            com = centroids[sid].copy()
            q = _random_rotation(rng)
            vel = np.array([rng.uniform(-1, 1), rng.uniform(-1, 1), rng.uniform(-2, 0)])
            ang = rng.uniform(-4, 4, 3)
            depth = rng.uniform(-0.05, 0.05)                  # lowest vertex this far below the ground (negative: above)
            gravity = True
            if cat == "force":
                weight = G / im
                for lo in (13, 16, 19):
                    if rng.random() < 0.75 or lo == 13 + 3 * (j % 3):
                        d = rng.normal(size=3)
                        b[lo:lo + 3] = d / np.linalg.norm(d) * weight * 10.0 ** rng.uniform(-3, 3) * (0.5 if lo > 13 else 1.0)
                gravity = j % 2 == 0
            elif cat == "asym_inertia" or cat == "ulp_shared":
                m = _asymmetric(rng, 6.0 * im)
                ang = rng.uniform(-8, 8, 3)
                b[16:19] = rng.normal(size=3) * 2.0 / im        # torques, so that integrate's M * torque is live too
                b[19:22] = rng.normal(size=3) * 2.0 / im
                depth = rng.uniform(0.0, 0.05)
            elif cat == "spd_inertia":
                m = _spd(rng, 6.0 * im)
                depth = rng.uniform(0.0, 0.05)
            elif cat == "static_linear":
                im = 0.0
                depth = rng.uniform(0.0, 0.05)
            elif cat == "mass_extreme":
                im = (1e-6, 1e6)[j % 2]
                m = m / m[0, 0] * (rng.uniform(2.0, 12.0) * (im if j % 4 < 2 else 1.0))
                depth = rng.uniform(0.0, 0.05)
            elif cat == "com_offset":
                com = rng.uniform(-1.0, 1.0, 3) * rng.uniform(0.5, 2.0)
            elif cat == "spin":
                axis = rng.normal(size=3)
                ang = axis / np.linalg.norm(axis) * rng.uniform(0.3, 1.0) * 2.0 / h      # h |w| / 2 up to 1
                m = _spd(rng, 30.0 * im) if j % 2 else _asymmetric(rng, 30.0 * im)
                depth = rng.uniform(0.05, 0.3)
            if cat == "ulp_shared":                             # every body of the shape: one static record
                srng = np.random.default_rng(seed + 7)
                im, m, com = 1.25, _asymmetric(srng, 7.5), centroids[sid].copy()
            b[0] = im
            set_matrix(b, m)
            if gravity:
                b[12] = -G / im if im > 0 else -G
            b[22:25], b[25:28], b[28:31], b[34:38] = vel, ang, com, q
            # position so that the lowest vertex of Rigid::frame() * vertex is at -depth
            local = np.array([_rotate(q, v - com) for v in verts[sid]])
            b[31] = PITCH * (k % 12)
            b[32] = PITCH * (k // 12)
            if cat == "far":
                b[31] += (1e4 if j % 2 else -1e4) + rng.uniform(-1, 1)
                b[32] += (-1e4 if j % 4 < 2 else 1e4) + rng.uniform(-1, 1)
            b[33] = -depth - local[:, 2].min() - com[2]
            rows.append(b)
            sids.append(sid)
            labels.append(cat)
            k += 1
    bodies = np.array(rows)
    ulp = [i for i, c in enumerate(labels) if c == "ulp_shared"]
    odd = ulp[len(ulp) // 2]
    bodies[odd, 2] = np.nextafter(bodies[odd, 2], np.inf)     # one ulp off in inverse_inertia column 0, row 1
    off = np.cumsum([0] + [len(v) for v in verts]).astype(np.uint32)
    return bodies, np.array(sids, dtype=np.uint32), np.concatenate(verts), off, np.array(labels)


def share_statics(bodies, shape_id):
    """Every body of a shape takes the static record (inverse mass, inverse inertia, centre of mass) of the shape's
    first body, bit for bit."""
    b = np.array(bodies, copy=True)
    for s in np.unique(shape_id):
        sel = np.nonzero(shape_id == s)[0]
        b[sel, 0:10] = b[sel[0], 0:10]
        b[sel, 28:31] = b[sel[0], 28:31]
    return b


EXACT_HEIGHTS = (0.0, -0.0, 2.0 ** -26, -2.0 ** -26, -2.0 ** -511, -2.0 ** -520, -2.0 ** -537, -2.0 ** -540, -5e-324)


def exact_heights():
    """The unit cube (vertex 0 at local (0,0,0), the bottom face in the plane z = 0), identity rotation, centre of mass at
    the origin, no force, sliding along x: the bottom face sits exactly at each height of EXACT_HEIGHTS.  Below 2^-511 the
    square in project_on is subnormal, below 2^-537.5 it is 0 and the reference returns NaN."""
    verts, _, _ = shapes()
    n = len(EXACT_HEIGHTS)
    b = np.zeros((2 * n, 38))
    b[:, 0] = 1.0
    b[:, 1:10] = np.eye(3).reshape(9) * 6.0
    b[:, 22] = 1.0                                      # tangential velocity
    b[:, 34] = 1.0
    b[:, 31] = PITCH * np.arange(2 * n)
    b[:n, 33] = EXACT_HEIGHTS
    b[n:, 33] = EXACT_HEIGHTS                           # the same heights with a spin about z: x, y move, z does not
    b[n:, 27] = 3.0
    sid = np.zeros(2 * n, dtype=np.uint32)
    labels = np.array(["height %r" % z for z in EXACT_HEIGHTS] * 2)
    return b, sid, verts[CUBE], np.array([0, 8], dtype=np.uint32), labels
