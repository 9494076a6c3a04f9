// xpbd_query_sweep.hip -- scene queries (EXTENSION) for gfx950: sweep queries, a convex volume cast along a segment against
// the world's bodies.  Staging, the line walk and the candidate walk are in xpbd_query_device.hpp.
#include "xpbd_query_units.hpp"

namespace xpbd {
namespace {

// ---- sweep queries: a convex volume translated along a segment -------------------------------------------------------------
// Semantics: include/xpbd.h, "Sweep queries".  The volume A at fa + t * d against the resting body B is, over every axis the SAT
// walks, one linear constraint "separation = s + t * v": the ray's slab test (ray_body) over the faces of A, the faces of B and
// both signs of every edge-direction pair.  The winner of a sweep is the minimum of its candidates under (t, index), and a
// candidate's t is a function of the sweep and the body alone, so neither the path nor how often a body is tested changes a bit.
static_assert(sizeof(xpbd_sweep) == 104 && sizeof(xpbd_sweep_hit) == 72, "xpbd_sweep is 104 bytes, xpbd_sweep_hit 72");
constexpr double kSweepMargin = 0.01; // the centre line is clipped to the grid's box grown by the radius and this part of a cell

struct Sweep {
    Frame f;
    Vec3 d;
    double tmax;
    uint32_t shape, ignore, mask;
};

__device__ __forceinline__ Sweep load_sweep(const xpbd_sweep *__restrict__ sweeps, uint32_t q)
{
    const xpbd_sweep &x = sweeps[q];
    return Sweep{Frame{Vec3{x.position[0], x.position[1], x.position[2]}, Quat{x.rotation[0], x.rotation[1], x.rotation[2], x.rotation[3]}},
                 Vec3{x.direction[0], x.direction[1], x.direction[2]}, x.max_distance, x.shape, x.ignore_body, x.mask};
}

// One lane per sweep: the bounding sphere of the volume at t = 0 (the layout of k_overlap_queries) and whether the sweep can hit
// anything -- a shape of the table, a finite frame and direction, a direction that moves, a max_distance >= 0 -- as radius >= 0.
__global__ void __launch_bounds__(kBlock) k_sweep_queries(const xpbd_sweep *__restrict__ sweeps, uint32_t n_sweeps, PolytopeTables t,
                                                          double *__restrict__ qrec)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_sweeps)
        return;
    const Sweep sw = load_sweep(sweeps, q);
    Vec3 c{0.0, 0.0, 0.0};
    double r = -1.0;
    if (sw.shape < t.n_shapes) {
        const double *cc = t.centroids + 3 * (size_t)sw.shape;
        c = sw.f * Vec3{cc[0], cc[1], cc[2]};
        const bool finite = isfinite(sw.f.position.x) && isfinite(sw.f.position.y) && isfinite(sw.f.position.z) && isfinite(sw.f.rotation.s) &&
                            isfinite(sw.f.rotation.x) && isfinite(sw.f.rotation.y) && isfinite(sw.f.rotation.z) && isfinite(c.x) &&
                            isfinite(c.y) && isfinite(c.z) && isfinite(sw.d.x) && isfinite(sw.d.y) && isfinite(sw.d.z);
        const bool moving = sw.d.x != 0.0 || sw.d.y != 0.0 || sw.d.z != 0.0;
        const double rs = t.radii[sw.shape];
        if (finite && moving && sw.tmax >= 0.0 && rs >= 0.0) // (a NaN max_distance fails the comparison; +inf passes)
            r = rs;
    }
    double2 *o = reinterpret_cast<double2 *>(qrec + (size_t)q * kOverlapRecDoubles);
    o[0] = double2{c.x, c.y};
    o[1] = double2{c.z, r};
}

// Conservative swept-sphere test: false only if the volume's bounding sphere, its centre moving from c along d over [0, t_end],
// certainly stays clear of the body's.  Never part of the definition: the slack (a relative 1e-6 on the reach, 1e-12 on the
// distance) is far above the rounding of the test and of the spheres, so no pair the routine below would hit is dropped.
__device__ __forceinline__ bool sweep_may_reach(Vec3 c, double rq, Vec3 d, double t_end, Vec3 cb, double rb)
{
    const Vec3 w = cb - c;
    const double reach = rq + rb;
    const double w2 = dot(w, w), wd = dot(w, d), dd = dot(d, d);
    const double bound = reach * reach * kSphereSlack + 1e-12 * w2;
    if (!(w2 > bound))
        return true; // in reach at the start
    if (wd < 0.0)
        return false; // out of reach and moving away
    const double ts = wd / dd;
    if (ts > t_end) { // the closest point of the segment is its end
        const Vec3 e = w - d * t_end;
        return !(dot(e, e) > bound);
    }
    return !(w2 - wd * ts > bound);
}

// The routine of one (sweep, body) pair by a group of L lanes.  A's world-space vertices are in s.world[0] already; t_cap is the
// sweep's max_distance or the best t so far, whichever is smaller (a pair that enters later cannot win, and an equal t still
// passes).  True on a hit, with its t and the position of the entering constraint in the order of the definition (kNoBody: the
// volume overlaps the body at the start).  Every lane of the group returns the same values.
template <uint32_t L, class Lds>
__device__ __forceinline__ bool sweep_decide(Lds &s, const PolytopeTables &t, const Frame &fa, const Frame &fa_inv, uint32_t sa, Vec3 d, Vec3 d_a,
                                             const Frame &fb, uint32_t sb, uint32_t lane, double t_cap, double &t_hit, uint32_t &entering)
{
    constexpr uint32_t H = L / 2;
    const ShapeDesc da = t.desc[sa], db = t.desc[sb];
    if (da.n_verts == 0 || db.n_verts == 0 || da.n_faces == 0 || db.n_faces == 0)
        return false;
    const Frame fb_inv = inverse(fb);
    const Vec3 d_b = fb_inv.rotation * d;
    const uint32_t half = lane / H, k = lane % H; // first half of the group works for A, second for B
    stage_pair(s, t, da, db, fa_inv, fb, fb_inv, half, k, H);

    double t_lo = -INFINITY, t_hi = t_cap;
    uint32_t enter = kNoBody;
    bool miss = false;
    // one constraint, position `at` in the order of the definition (ascending on every lane: the first maximum stays)
    auto constrain = [&](double sep, double vel, uint32_t at) {
        if (sep != sep || vel != vel) {
            miss = true;
        } else if (vel < 0.0) {
            const double tk = (-sep) / vel;
            if (tk > t_lo) {
                t_lo = tk;
                enter = at;
            }
        } else if (vel > 0.0) {
            const double tk = (-sep) / vel;
            t_hi = tk < t_hi ? tk : t_hi;
        } else if (sep >= 0.0) {
            miss = true;
        }
    };
    // the group's t_lo (first maximum), t_hi and verdict so far; true: a miss for good
    auto settle = [&]() -> bool {
        reduce_max_first(t_lo, enter, L);
        for (uint32_t off = L >> 1; off; off >>= 1) {
            const double o = partner(t_hi, off);
            t_hi = o < t_hi ? o : t_hi;
        }
        return group_bits<L>(__ballot(miss)) != 0 || t_lo > t_hi;
    };

    // ---- faces: A's on the first half (against B's vertices in A's space), B's on the second ------------------------------
    {
        const ShapeDesc dm = half ? db : da;
        const uint32_t n_other = half ? da.n_verts : db.n_verts;
        const Vec3 d_m = half ? d_b : d_a;
        for (uint32_t f = k; f < dm.n_faces; f += H) {
            const double *pl = t.planes + 4 * (size_t)(dm.face0 + f);
            const Vec3 n{pl[0], pl[1], pl[2]};
            double low = dot(n, ld3(s.local[half ^ 1u], 0));
            for (uint32_t v = 1; v < n_other; ++v) {
                const double x = dot(n, ld3(s.local[half ^ 1u], v));
                low = x < low ? x : low;
            }
            const double w = dot(n, d_m);
            constrain(low - pl[3], half ? w : -w, half ? da.n_faces + f : f);
        }
    }
    if (settle())
        return false;

    // ---- edge axes: (unique edge direction of A) x (unique edge direction of B), both signs -------------------------------
    const bool dirs_staged = stage_edge_dirs<L>(s, t, da, db, fa, fb, lane);
    const uint32_t total = da.n_dirs * db.n_dirs, edge0 = da.n_faces + db.n_faces;
    for (uint32_t q = lane; q < total; q += L) {
        const uint32_t i = q / db.n_dirs, j = q - i * db.n_dirs;
        const Vec3 n = edge_axis(s, dirs_staged, t, da, db, fa, fb, i, j);
        if (!(fabs(n.x) <= DBL_MAX && fabs(n.y) <= DBL_MAX && fabs(n.z) <= DBL_MAX))
            continue; // parallel directions: no axis
        double hi_a = dot(ld3(s.world[0], 0), n), lo_a = hi_a, hi_b = dot(ld3(s.world[1], 0), n), lo_b = hi_b;
        for (uint32_t v = 1; v < da.n_verts; ++v) {
            const double x = dot(ld3(s.world[0], v), n);
            hi_a = x > hi_a ? x : hi_a;
            lo_a = x < lo_a ? x : lo_a;
        }
        for (uint32_t v = 1; v < db.n_verts; ++v) {
            const double x = dot(ld3(s.world[1], v), n);
            hi_b = x > hi_b ? x : hi_b;
            lo_b = x < lo_b ? x : lo_b;
        }
        const double w = dot(n, d);
        constrain(lo_b - hi_a, -w, edge0 + 2u * q);
        constrain(lo_a - hi_b, w, edge0 + 2u * q + 1u);
    }
    if (settle())
        return false;
    const bool initial = t_lo < 0.0;
    t_hit = initial ? 0.0 : t_lo;
    entering = initial ? kNoBody : enter;
    return t_hit <= t_hi;
}

struct SweepArgs : PassArgs {
    const xpbd_sweep *sweeps;
    xpbd_sweep_hit *hits;
};

// The closest body of every sweep: one group of L lanes per sweep, 64 / L sweeps per wave.  The lanes of a group admit one
// candidate each (ignore_body, the mask, the swept spheres) and the group then decides the survivors one after the other.  On
// the grid path the centre line is walked cell by cell as k_query_walk walks a ray, and for the time the centre spends in one
// cell the lanes share out the box of cells the volume's sphere covers meanwhile.
template <uint32_t L, uint32_t V>
__global__ void __launch_bounds__(64) k_sweep_pass(BodyArrays b, PolytopeTables t, SweepArgs a)
{
    constexpr uint32_t PW = 64 / L;
    __shared__ OverlapLds<V> s_all[PW];
    const uint32_t group = threadIdx.x / L, lane = threadIdx.x % L;
    const uint32_t q = blockIdx.x * PW + group;
    if (q >= a.n)
        return;
    OverlapLds<V> &s = s_all[group];
    const double2 *qr = reinterpret_cast<const double2 *>(a.qrec + (size_t)q * kOverlapRecDoubles);
    const double2 q0 = qr[0], q1 = qr[1];
    const Vec3 cq{q0.x, q0.y, q1.x};
    const double rq = q1.y;
    const Sweep sw = load_sweep(a.sweeps, q);
    Best best = no_hit(); // (face: the position of the entering constraint)
    Frame fq_inv{};
    Vec3 d_q{0.0, 0.0, 0.0};
    if (rq >= 0.0) {
        fq_inv = inverse(sw.f);
        d_q = fq_inv.rotation * sw.d;
        {
            const ShapeDesc dq = t.desc[sw.shape];
            for (uint32_t vtx = lane; vtx < dq.n_verts; vtx += L) {
                const double *v = t.verts + 3 * (size_t)(dq.vert0 + vtx);
                st3(s.world[0], vtx, sw.f * Vec3{v[0], v[1], v[2]});
            }
        }
        // may body i win? (one lane)
        auto admit = [&](uint32_t i, Vec3 &centre, double &radius) -> bool {
            return admit_record(a, i, sw.ignore, sw.mask, centre, radius) &&
                   sweep_may_reach(cq, rq, sw.d, best.t < sw.tmax ? best.t : sw.tmax, centre, radius);
        };
        // the bodies the lanes of the group hold in `mine`
        auto decide = [&](uint32_t mine) {
            for_each_held<L>(mine, [&](uint32_t i) {
                double th = 0.0;
                uint32_t entering = kNoBody;
                if (sweep_decide<L>(s, t, sw.f, fq_inv, sw.shape, sw.d, d_q, body_frame(b, i), b.shape_id[i], lane,
                                    best.t < sw.tmax ? best.t : sw.tmax, th, entering)) {
                    const uint32_t id = a.gid ? a.gid[i] : i;
                    if (better(th, id, best))
                        best = Best{th, id, entering, i, 0};
                }
            });
        };
        QueryGrid g{};
        if (!a.brute)
            g = *a.grid;
        if (a.brute || g.mode == kEveryBody || (g.mode == kGrid && !(rq <= kSweepReach * g.edge))) {
            for (uint32_t i0 = 0; i0 < b.n; i0 += L) {
                const uint32_t i = i0 + lane;
                Vec3 cb;
                double rb;
                decide(i < b.n && admit(i, cb, rb) ? i : kNoBody);
            }
        } else if (g.mode == kGrid) {
            const double o[3] = {cq.x, cq.y, cq.z}, d[3] = {sw.d.x, sw.d.y, sw.d.z};
            // clip the centre line to the grid's box grown by the volume's radius: [t_near, t_far].  Outside it the volume
            // reaches no body's sphere; the cells of the walk may lie outside the grid, the boxes below are clamped to it.
            double t_near, t_far;
            if (clip_to_grid(g, o, d, sw.tmax, rq + kSweepMargin * g.edge, t_near, t_far)) {
                int32_t cell[3], step[3];
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    const double p = d[ax] == 0.0 ? o[ax] : o[ax] + t_near * d[ax];
                    // (within kSweepReach + 1 cells of the grid, by the clip; the bound keeps the conversion defined regardless)
                    double c = floor(p / g.edge);
                    const double c_lo = (double)g.lo[ax] - (kSweepReach + 2.0), c_hi = (double)g.lo[ax] + (double)g.dims[ax] + (kSweepReach + 2.0);
                    c = c < c_lo ? c_lo : (c > c_hi ? c_hi : c);
                    cell[ax] = (int32_t)c;
                    step[ax] = d[ax] > 0.0 ? 1 : (d[ax] < 0.0 ? -1 : 0);
                }
                double t_enter = t_near;
                // the previous stretch's box; none yet: empty whatever the sign of the grid's cell coordinates
                int32_t plo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, phi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
                for (;;) {
                    if (t_enter > best.t) // strict: a tie later on can still win on the smaller index
                        break;
                    // when the centre leaves this cell
                    double t_next;
                    const int axis = next_face(g, cell, step, o, d, t_next);
                    const double t_leave = t_next < t_far ? t_next : t_far;
                    // the box of cells the sphere covers while its centre runs over [t_enter, t_leave]
                    int32_t qlo[3];
                    uint32_t qdim[3];
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        const double p0 = d[ax] == 0.0 ? o[ax] : o[ax] + t_enter * d[ax], p1 = d[ax] == 0.0 ? o[ax] : o[ax] + t_leave * d[ax];
                        const double c_min = p0 < p1 ? p0 : p1, c_max = p0 < p1 ? p1 : p0;
                        qlo[ax] = clamp_axis(g, ax, floor((c_min - rq - g.pad) / g.edge));
                        const int32_t hi = clamp_axis(g, ax, floor((c_max + rq + g.pad) / g.edge));
                        qdim[ax] = (uint32_t)(hi - qlo[ax]) + 1u;
                    }
                    // A body counts in one cell of this box (walk_cell_box), and not at all if the previous stretch's box held
                    // one of its cells -- the boxes that meet a body's cells are consecutive stretches (the centre moves one
                    // way on every axis), so it was looked at then, with a t_cap no smaller than now.  A test too many would
                    // change nothing.
                    walk_cell_box<L>(g, qlo, qdim, a.cell_start, a.items, lane, admit,
                                     [&](int ax, int32_t lo, int32_t hi) { return lo <= phi[ax] && hi >= plo[ax]; }, decide);
                    if (axis < 0 || t_next > t_far)
                        break;
#pragma unroll
                    for (int ax = 0; ax < 3; ++ax) {
                        plo[ax] = qlo[ax];
                        phi[ax] = qlo[ax] + (int32_t)qdim[ax] - 1;
                    }
                    cell[axis] += step[axis];
                    t_enter = t_next;
                }
            }
        }
    }
    if (lane != 0)
        return;
    xpbd_sweep_hit h;
    h.body = best.id;
    h.feature = 0;
    h.face = XPBD_NO_HIT;
    h.reserved = 0;
    h.distance = INFINITY;
    h.position[0] = h.position[1] = h.position[2] = 0.0;
    h.normal[0] = h.normal[1] = h.normal[2] = 0.0;
    if (best.id != XPBD_NO_HIT) {
        h.distance = best.t;
        const Vec3 p = sw.f.position + sw.d * best.t;
        h.position[0] = p.x, h.position[1] = p.y, h.position[2] = p.z;
        const uint32_t sb = b.shape_id[best.slot];
        const ShapeDesc da = t.desc[sw.shape], db = t.desc[sb];
        const uint32_t at = best.face;
        if (at == kNoBody) {
            h.feature = XPBD_SWEEP_INITIAL;
        } else {
            const Frame fb = body_frame(b, best.slot);
            Vec3 n;
            if (at < da.n_faces) {
                const double *pl = t.planes + 4 * (size_t)(da.face0 + at);
                h.feature = XPBD_FEATURE_FACE_A;
                h.face = at;
                n = -(sw.f.rotation * Vec3{pl[0], pl[1], pl[2]});
            } else if (at < da.n_faces + db.n_faces) {
                const double *pl = t.planes + 4 * (size_t)(db.face0 + (at - da.n_faces));
                h.feature = XPBD_FEATURE_FACE_B;
                h.face = at - da.n_faces;
                n = fb.rotation * Vec3{pl[0], pl[1], pl[2]};
            } else {
                const uint32_t e = at - da.n_faces - db.n_faces, pair = e >> 1, i = pair / db.n_dirs, j = pair - i * db.n_dirs;
                n = edge_axis_of_table(t, da, db, sw.f, fb, i, j);
                h.feature = XPBD_FEATURE_EDGES;
                n = (e & 1u) ? n : -n;
            }
            h.normal[0] = n.x, h.normal[1] = n.y, h.normal[2] = n.z;
        }
    }
    a.hits[q] = h;
}

} // namespace

hipError_t launch_sweep(const BodyArrays &b, const PolytopeTables &t, const uint32_t *global_id, const uint2 *filter, const void *sweeps_v,
                        uint32_t n_sweeps, bool masked, bool brute, const QueryScratch &s, void *hits_v, hipStream_t stream, const Terrain *terrain,
                        bool terrain_brute)
{
    if (n_sweeps == 0)
        return hipSuccess;
    brute = brute || b.n == 0;
    const xpbd_sweep *sweeps = static_cast<const xpbd_sweep *>(sweeps_v);
    launch_query_bodies(b, t, global_id, RayFilter{nullptr, 0u, 0u}, s, stream);
    hipLaunchKernelGGL(k_sweep_queries, dim3(blocks_of(n_sweeps)), dim3(kBlock), 0, stream, sweeps, n_sweeps, t, s.qrec);
    if (!brute)
        if (hipError_t e = launch_query_grid(b, s, stream)) // the grid of a ray cast, by the same passes
            return e;
    const SweepArgs a{pass_args(s, global_id, filter, n_sweeps, masked, brute), sweeps, static_cast<xpbd_sweep_hit *>(hits_v)};
    with_group_shape(t, n_sweeps, [&](auto l, auto v, dim3 blocks) {
        hipLaunchKernelGGL((k_sweep_pass<decltype(l)::value, decltype(v)::value>), blocks, dim3(64), 0, stream, b, t, a);
    });
    const hipError_t e = hipGetLastError();
    return e != hipSuccess || !terrain ? e : launch_terrain_sweeps(*terrain, t, sweeps_v, n_sweeps, terrain_brute, s.qrec, hits_v, stream);
}

} // namespace xpbd
