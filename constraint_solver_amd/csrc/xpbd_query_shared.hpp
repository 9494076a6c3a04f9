// xpbd_query_shared.hpp -- the routines of one candidate that more than one scene-query unit runs: the ray-body rule and the
// distance query's vertex-over-face and clamped-segment candidates (include/xpbd.h, "Scene queries", "Distance queries").
// xpbd_query.hip runs them against the bodies, xpbd_terrain_query.hip against the heightfield; one definition, so the same
// bits.  Host code too (XPBD_HD): a CPU program can run the terrain distance walk against its brute force.
#pragma once

#include <cmath>
#include <cstdint>

#include "xpbd_internal.h"
#include "xpbd_math.hpp"
#include "xpbd_pairs.h"

namespace xpbd {

// The sphere pre-test rejects a body only when the ray's line passes farther than its sphere by a relative 1e-6 (a few
// thousand times the rounding of the test): it never decides a hit, only saves the face loop of bodies the ray cannot reach.
constexpr double kSphereSlack = 1.0 + 1e-6;

struct Ray {
    Vec3 o, d;
    double tmax;
    uint32_t ignore;
    bool valid;
};

struct BodyQ {
    Vec3 inv_pos;
    Quat inv_rot;
    Vec3 centre;
    double radius; // < 0: never hit
};

// The routine of one (ray, body) pair (include/xpbd.h): true on a hit, with its t and entering face.
XPBD_HD bool ray_body(const Ray &ray, const BodyQ &q, const PolytopeTables &t, uint32_t sid, double &t_hit,
                                         uint32_t &face)
{
    const Vec3 o_l = q.inv_rot * ray.o + q.inv_pos; // inv * origin (src/frame.rs:47-53)
    const Vec3 d_l = q.inv_rot * ray.d;
    const ShapeDesc desc = t.desc[sid];
    double t_lo = 0.0, t_hi = ray.tmax;
    uint32_t f = XPBD_RAY_INSIDE;
    for (uint32_t k = 0; k < desc.n_faces; ++k) {
        const double *p = t.planes + 4 * (size_t)(desc.face0 + k);
        const Plane pl{Vec3{p[0], p[1], p[2]}, p[3]};
        const double s = distance(pl, o_l), v = dot(pl.normal, d_l);
        if (s != s || v != v)
            return false;
        if (v < 0.0) {
            const double tk = (-s) / v;
            if (tk > t_lo) {
                t_lo = tk;
                f = k;
            }
        } else if (v > 0.0) {
            const double tk = (-s) / v;
            t_hi = tk < t_hi ? tk : t_hi;
        } else if (s > 0.0) {
            return false;
        }
        if (t_lo > t_hi) // t_lo only grows and t_hi only shrinks: a miss for good
            return false;
    }
    t_hit = t_lo;
    face = f;
    return true;
}

// "x lies in face F" of the definition: `face` counts over all shapes, vert0 is the shape's first vertex, n the face's normal.
XPBD_HD bool lies_in_face(const PolytopeTables &t, uint32_t vert0, uint32_t face, Vec3 n, Vec3 x)
{
    const uint32_t f0 = t.face_start[face], m = t.face_start[face + 1] - f0;
    const uint32_t *fv = t.face_verts + f0;
    auto vert = [&](uint32_t k) {
        const double *v = t.verts + 3 * (size_t)(vert0 + fv[k]);
        return Vec3{v[0], v[1], v[2]};
    };
    bool in = true;
    for (uint32_t k = 0; k < m && in; ++k) {
        const uint32_t k1 = k + 1 < m ? k + 1 : k + 1 - m, k2 = k + 2 < m ? k + 2 : k + 2 - m;
        const Vec3 a = vert(k), b = vert(k1), c = vert(k2);
        Vec3 side = cross(b - a, n);
        if (dot(side, c - a) > 0.0)
            side = -side;
        in = dot(side, x - a) <= 0.0;
    }
    return in;
}

// A vertex at p (in the face's local space) over face `face`: true if the candidate counts and its d2 = h * h lies below `below`
// (a candidate that does not cannot replace the best so far: its foot is not looked at), with h and the foot.
XPBD_HD bool vertex_over_face(const PolytopeTables &t, uint32_t vert0, uint32_t face, Vec3 p, double below, double &h, Vec3 &foot)
{
    const double *pl = t.planes + 4 * (size_t)face;
    const Vec3 n{pl[0], pl[1], pl[2]};
    h = dot(n, p) - pl[3];
    if (!(h >= 0.0) || !(h * h < below))
        return false;
    foot = p - h * n;
    return lies_in_face(t, vert0, face, n, foot);
}

XPBD_HD double clamp01(double x) { return x < 0.0 ? 0.0 : (x > 1.0 ? 1.0 : x); }

// The clamped closest points of the segments P0 P1 and Q0 Q1, branch by branch as the definition lists them: d2, and the points.
XPBD_HD double segment_closest(Vec3 p0, Vec3 p1, Vec3 q0, Vec3 q1, Vec3 &ca, Vec3 &cb)
{
    const Vec3 u = p1 - p0, w = q1 - q0, r = p0 - q0;
    const double a = dot(u, u), e = dot(w, w), f = dot(w, r);
    double s = 0.0, tt = 0.0;
    if (a == 0.0 && e == 0.0) {
    } else if (a == 0.0) {
        tt = clamp01(f / e);
    } else {
        const double c = dot(u, r);
        if (e == 0.0) {
            s = clamp01((-c) / a);
        } else {
            const double b = dot(u, w), den = a * e - b * b;
            s = den > 0.0 ? clamp01((b * f - c * e) / den) : 0.0;
            tt = (b * s + f) / e;
            if (tt < 0.0) {
                tt = 0.0;
                s = clamp01((-c) / a);
            } else if (tt > 1.0) {
                tt = 1.0;
                s = clamp01((b - c) / a);
            }
        }
    }
    ca = p0 + u * s;
    cb = q0 + w * tt;
    const Vec3 g = ca - cb;
    return dot(g, g);
}

} // namespace xpbd
