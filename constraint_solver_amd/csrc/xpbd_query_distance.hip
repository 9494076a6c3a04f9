// xpbd_query_distance.hip -- scene queries (EXTENSION) for gfx950: distance queries, the body nearest to a convex volume or a
// point.  The overlap query's decision, staging and the candidate walk are in xpbd_query_device.hpp.
#include "xpbd_query_units.hpp"

namespace xpbd {
namespace {

// ---- distance queries: the body nearest to a convex volume or a point -------------------------------------------------------
// Semantics: include/xpbd.h, "Distance queries".  One (volume, body) pair is the overlap query's decision first and then the
// minimum of d2 over a fixed list of candidates -- vertex over face both ways, then every pair of edges -- under (d2, position in
// the list).  A pair's distance is a function of the query and the body alone and the winner of a query is the minimum under
// (distance, index), so neither the path nor how often a body is looked at changes a bit.
static_assert(sizeof(xpbd_distance_query) == 80 && sizeof(xpbd_distance_hit) == 96, "xpbd_distance_query is 80 bytes, xpbd_distance_hit 96");
constexpr uint32_t kOverlapAt = 0xFFFFFFFEu; // Best::face of a pair that is not separated (kNoBody: no candidate)

struct DistanceQ {
    Frame f;
    double dmax;
    uint32_t shape, ignore, mask;
};

__device__ __forceinline__ DistanceQ load_distance(const xpbd_distance_query *__restrict__ queries, uint32_t q)
{
    const xpbd_distance_query &x = queries[q];
    return DistanceQ{Frame{Vec3{x.position[0], x.position[1], x.position[2]}, Quat{x.rotation[0], x.rotation[1], x.rotation[2], x.rotation[3]}},
                     x.max_distance, x.shape, x.ignore_body, x.mask};
}

// The volume's shape as the candidate lists see it: the point volume is one vertex, no faces and one edge from it to itself.
__device__ __forceinline__ ShapeDesc volume_desc(const PolytopeTables &t, uint32_t shape)
{
    return shape == XPBD_DISTANCE_POINT ? ShapeDesc{0, 1, 0, 0, 0, 1, 0, 0} : t.desc[shape];
}

// One lane per query: the bounding sphere of the volume (the layout of k_overlap_queries; the point volume: its position, radius
// 0) and whether the query can find anything -- a shape of the table or the point, a finite frame, a max_distance >= 0 -- as
// radius >= 0.
__global__ void __launch_bounds__(kBlock) k_distance_queries(const xpbd_distance_query *__restrict__ queries, uint32_t n_queries, PolytopeTables t,
                                                             double *__restrict__ qrec)
{
    const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n_queries)
        return;
    const DistanceQ dq = load_distance(queries, q);
    const bool point = dq.shape == XPBD_DISTANCE_POINT;
    Vec3 c{0.0, 0.0, 0.0};
    double r = -1.0;
    if (point || dq.shape < t.n_shapes) {
        c = dq.f.position;
        double rs = 0.0;
        if (!point) {
            const double *cc = t.centroids + 3 * (size_t)dq.shape;
            c = dq.f * Vec3{cc[0], cc[1], cc[2]};
            rs = t.radii[dq.shape];
        }
        const bool finite = isfinite(dq.f.position.x) && isfinite(dq.f.position.y) && isfinite(dq.f.position.z) && isfinite(dq.f.rotation.s) &&
                            isfinite(dq.f.rotation.x) && isfinite(dq.f.rotation.y) && isfinite(dq.f.rotation.z) && isfinite(c.x) &&
                            isfinite(c.y) && isfinite(c.z);
        if (finite && dq.dmax >= 0.0 && rs >= 0.0) // (a NaN max_distance fails the comparison; +inf passes)
            r = rs;
    }
    double2 *o = reinterpret_cast<double2 *>(qrec + (size_t)q * kOverlapRecDoubles);
    o[0] = double2{c.x, c.y};
    o[1] = double2{c.z, r};
}

// The routine of one (volume, body) pair by a group of L lanes.  A's world-space vertices are in s.world[0] already.  True if
// the pair has an answer at all: its distance and `at`, the position of the winning candidate in the order of the definition
// (kOverlapAt: not separated).  Every lane of the group returns the same values.
template <uint32_t L, class Lds>
__device__ __forceinline__ bool distance_decide(Lds &s, const PolytopeTables &t, const Frame &fa, const Frame &fa_inv, uint32_t sa, const Frame &fb,
                                                uint32_t sb, bool spheres, uint32_t lane, double &dist, uint32_t &at)
{
    constexpr uint32_t H = L / 2;
    const bool point = sa == XPBD_DISTANCE_POINT;
    const ShapeDesc da = volume_desc(t, sa), db = t.desc[sb];
    if (da.n_verts == 0 || db.n_verts == 0)
        return false;
    // ---- 1. the overlap query's decision --------------------------------------------------------------------------------
    if (spheres && !point) {
        uint32_t feature = 0;
        double separation = 0.0;
        if (overlap_decide<L>(s, t, fa, fa_inv, sa, fb, sb, lane, feature, separation)) {
            dist = 0.0;
            at = kOverlapAt;
            return true;
        }
    }
    // (again after a SAT that got as far as its edge axes: those may stand where the vertices stood)
    const Frame fb_inv = inverse(fb);
    stage_pair(s, t, da, db, fa_inv, fb, fb_inv, lane / H, lane % H, H);
    if (spheres && point && db.n_faces) {
        const Vec3 p = ld3(s.local[0], 0);
        const double *pl = t.planes + 4 * (size_t)db.face0;
        double deepest = dot(Vec3{pl[0], pl[1], pl[2]}, p) - pl[3];
        for (uint32_t f = 1; f < db.n_faces; ++f) {
            pl += 4;
            const double x = dot(Vec3{pl[0], pl[1], pl[2]}, p) - pl[3];
            deepest = x > deepest ? x : deepest;
        }
        if (deepest < 0.0) {
            dist = 0.0;
            at = kOverlapAt;
            return true;
        }
    }
    // ---- 2 (a), (b): vertex over face, A's vertices over B's faces and then B's over A's, spread over the lanes ---------------
    double d2 = INFINITY;
    at = kNoBody;
    const uint32_t over_b = da.n_verts * db.n_faces, faces = over_b + db.n_verts * da.n_faces;
    for (uint32_t c = lane; c < faces; c += L) {
        const bool on_b = c < over_b;
        const uint32_t cc = on_b ? c : c - over_b, nf = on_b ? db.n_faces : da.n_faces;
        const uint32_t v = cc / nf, f = cc - v * nf;
        double h;
        Vec3 foot;
        if (vertex_over_face(t, on_b ? db.vert0 : da.vert0, (on_b ? db.face0 : da.face0) + f, ld3(s.local[on_b ? 0 : 1], v), d2, h, foot)) {
            d2 = h * h; // ascending c on this lane: the first minimum stays
            at = c;
        }
    }
    reduce_min_first(d2, at, L);
    // ---- 2 (c): every edge of A against every edge of B, spread over the lanes, from the faces' winner on -----------------
    const uint32_t pairs = da.n_edges * db.n_edges;
    for (uint32_t q = lane; q < pairs; q += L) {
        const uint32_t i = q / db.n_edges, j = q - i * db.n_edges;
        const uint32_t *eb = t.edges + 2 * (size_t)(db.edge0 + j);
        uint32_t a0 = 0, a1 = 0;
        if (!point) {
            const uint32_t *ea = t.edges + 2 * (size_t)(da.edge0 + i);
            a0 = ea[0], a1 = ea[1];
        }
        Vec3 ca, cb;
        const double x = segment_closest(ld3(s.world[0], a0), ld3(s.world[0], a1), ld3(s.world[1], eb[0]), ld3(s.world[1], eb[1]), ca, cb);
        if (x < d2) {
            d2 = x;
            at = faces + q;
        }
    }
    reduce_min_first(d2, at, L);
    if (at == kNoBody)
        return false;
    dist = sqrt(d2);
    return true;
}

struct DistanceArgs : PassArgs {
    const xpbd_distance_query *queries;
    xpbd_distance_hit *hits;
};

// The nearest body of every query: one group of L lanes per query, 64 / L queries per wave.  The lanes of a group admit one
// candidate each (ignore_body, the mask, the gap between the bounding spheres against min(max_distance, best so far)) and the
// group then decides the survivors one after the other.  On the grid path the lanes share out the cells the volume's sphere
// covers, then those the sphere grown by min(max_distance, best so far) covers beyond them.
template <uint32_t L, uint32_t V>
__global__ void __launch_bounds__(64) k_distance_pass(BodyArrays b, PolytopeTables t, DistanceArgs a)
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
    const DistanceQ dq = load_distance(a.queries, q);
    const bool point = dq.shape == XPBD_DISTANCE_POINT;
    Best best = no_hit(); // (face: the position of the winning candidate)
    Frame fq_inv{};
    if (rq >= 0.0) {
        fq_inv = inverse(dq.f);
        if (point) {
            if (lane == 0)
                st3(s.world[0], 0, dq.f.position);
        } else {
            const ShapeDesc ds = t.desc[dq.shape];
            for (uint32_t vtx = lane; vtx < ds.n_verts; vtx += L) {
                const double *v = t.verts + 3 * (size_t)(ds.vert0 + vtx);
                st3(s.world[0], vtx, dq.f * Vec3{v[0], v[1], v[2]});
            }
        }
        // may body i win? (one lane)  Conservative: the gap between the spheres is a lower bound of the distance, and the sweep
        // pre-test's slack is far above the rounding of the test and of the spheres.  Never part of the definition.
        auto admit = [&](uint32_t i, Vec3 &centre, double &radius) -> bool {
            if (!admit_record(a, i, dq.ignore, dq.mask, centre, radius))
                return false;
            const Vec3 w = centre - cq;
            const double w2 = dot(w, w), reach = rq + radius + (best.t < dq.dmax ? best.t : dq.dmax);
            return !(w2 > reach * reach * kSphereSlack + 1e-12 * w2);
        };
        // the bodies the lanes of the group hold in `mine`
        auto decide = [&](uint32_t mine) {
            for_each_held<L>(mine, [&](uint32_t i) {
                double dist = 0.0;
                uint32_t at = kNoBody;
                if (distance_decide<L>(s, t, dq.f, fq_inv, dq.shape, body_frame(b, i), b.shape_id[i], spheres_overlap(a.rec, i, cq, rq), lane, dist,
                                       at) &&
                    dist <= dq.dmax) {
                    const uint32_t id = a.gid ? a.gid[i] : i;
                    if (better(dist, id, best))
                        best = Best{dist, id, at, i, 0};
                }
            });
        };
        QueryGrid g{};
        if (!a.brute)
            g = *a.grid;
        if (a.brute || g.mode == kEveryBody || (g.mode == kGrid && !(rq + dq.dmax <= kSweepReach * g.edge))) {
            for (uint32_t i0 = 0; i0 < b.n; i0 += L) {
                const uint32_t i = i0 + lane;
                Vec3 cb;
                double rb;
                decide(i < b.n && admit(i, cb, rb) ? i : kNoBody);
            }
        } else if (g.mode == kGrid) {
            const double c[3] = {cq.x, cq.y, cq.z};
            // the box of cells a sphere of radius `reach` about the volume's centre covers (at most 2 kSweepReach + 2 cells a side:
            // fewer than the smallest table has keys)
            auto cells_of = [&](double reach, int32_t(&lo)[3], uint32_t(&dim)[3]) {
#pragma unroll
                for (int ax = 0; ax < 3; ++ax) {
                    lo[ax] = clamp_axis(g, ax, floor((c[ax] - reach - g.pad) / g.edge));
                    const int32_t hi = clamp_axis(g, ax, floor((c[ax] + reach + g.pad) / g.edge));
                    dim[ax] = (uint32_t)(hi - lo[ax]) + 1u;
                }
            };
            int32_t plo[3], qlo[3];
            uint32_t pdim[3], qdim[3];
            cells_of(rq, plo, pdim);
            walk_cell_box<L>(g, plo, pdim, a.cell_start, a.items, lane, admit, [](int, int32_t, int32_t) { return false; }, decide);
            // A body whose cells met the first box was looked at there, with a bound no smaller than now: not again.
            cells_of(rq + (best.t < dq.dmax ? best.t : dq.dmax), qlo, qdim);
            if (qdim[0] != pdim[0] || qdim[1] != pdim[1] || qdim[2] != pdim[2])
                walk_cell_box<L>(g, qlo, qdim, a.cell_start, a.items, lane, admit,
                                 [&](int ax, int32_t lo, int32_t hi) { return lo <= plo[ax] + (int32_t)pdim[ax] - 1 && hi >= plo[ax]; }, decide);
        }
    }
    if (lane != 0)
        return;
    xpbd_distance_hit h;
    h.body = best.id;
    h.feature = 0;
    h.index_a = h.index_b = XPBD_NO_HIT;
    h.distance = INFINITY;
    h.point_a[0] = h.point_a[1] = h.point_a[2] = 0.0;
    h.point_b[0] = h.point_b[1] = h.point_b[2] = 0.0;
    h.normal[0] = h.normal[1] = h.normal[2] = 0.0;
    if (best.id != XPBD_NO_HIT) {
        h.distance = best.t;
        if (best.face == kOverlapAt) {
            h.feature = XPBD_DISTANCE_OVERLAP;
        } else {
            // the winning candidate once more, by the expressions that staged and measured it
            const uint32_t sb = b.shape_id[best.slot];
            const ShapeDesc da = volume_desc(t, dq.shape), db = t.desc[sb];
            const Frame fb = body_frame(b, best.slot), fb_inv = inverse(fb);
            auto world_a = [&](uint32_t v) {
                if (point)
                    return dq.f.position;
                const double *x = t.verts + 3 * (size_t)(da.vert0 + v);
                return dq.f * Vec3{x[0], x[1], x[2]};
            };
            auto world_b = [&](uint32_t v) {
                const double *x = t.verts + 3 * (size_t)(db.vert0 + v);
                return fb * Vec3{x[0], x[1], x[2]};
            };
            const uint32_t over_b = da.n_verts * db.n_faces, faces = over_b + db.n_verts * da.n_faces, at = best.face;
            Vec3 pa{0.0, 0.0, 0.0}, pb{0.0, 0.0, 0.0}, foot{0.0, 0.0, 0.0};
            double hh = 0.0;
            if (at < over_b) {
                const uint32_t v = at / db.n_faces, f = at - v * db.n_faces;
                pa = world_a(v);
                vertex_over_face(t, db.vert0, db.face0 + f, fb_inv * pa, INFINITY, hh, foot);
                pb = fb * foot;
                h.feature = XPBD_FEATURE_FACE_B, h.index_a = v, h.index_b = f;
            } else if (at < faces) {
                const uint32_t v = (at - over_b) / da.n_faces, f = (at - over_b) - v * da.n_faces;
                pb = world_b(v);
                vertex_over_face(t, da.vert0, da.face0 + f, fq_inv * pb, INFINITY, hh, foot);
                pa = dq.f * foot;
                h.feature = XPBD_FEATURE_FACE_A, h.index_a = f, h.index_b = v;
            } else {
                const uint32_t e = at - faces, i = e / db.n_edges, j = e - i * db.n_edges;
                const uint32_t *eb = t.edges + 2 * (size_t)(db.edge0 + j);
                uint32_t a0 = 0, a1 = 0;
                if (!point) {
                    const uint32_t *ea = t.edges + 2 * (size_t)(da.edge0 + i);
                    a0 = ea[0], a1 = ea[1];
                }
                segment_closest(world_a(a0), world_a(a1), world_b(eb[0]), world_b(eb[1]), pa, pb);
                h.feature = XPBD_FEATURE_EDGES, h.index_a = i, h.index_b = j;
            }
            h.point_a[0] = pa.x, h.point_a[1] = pa.y, h.point_a[2] = pa.z;
            h.point_b[0] = pb.x, h.point_b[1] = pb.y, h.point_b[2] = pb.z;
            if (best.t != 0.0) {
                const Vec3 n = (pa - pb) * (1.0 / best.t);
                h.normal[0] = n.x, h.normal[1] = n.y, h.normal[2] = n.z;
            }
        }
    }
    a.hits[q] = h;
}

} // namespace

hipError_t launch_distance(const BodyArrays &b, const PolytopeTables &t, const uint32_t *global_id, const uint2 *filter, const void *queries_v,
                           uint32_t n_queries, bool masked, bool brute, const QueryScratch &s, void *hits_v, hipStream_t stream)
{
    if (n_queries == 0)
        return hipSuccess;
    brute = brute || b.n == 0;
    const xpbd_distance_query *queries = static_cast<const xpbd_distance_query *>(queries_v);
    launch_query_bodies(b, t, global_id, RayFilter{nullptr, 0u, 0u}, s, stream);
    hipLaunchKernelGGL(k_distance_queries, dim3(blocks_of(n_queries)), dim3(kBlock), 0, stream, queries, n_queries, t, s.qrec);
    if (!brute)
        if (hipError_t e = launch_query_grid(b, s, stream)) // the grid of a ray cast, by the same passes
            return e;
    const DistanceArgs a{pass_args(s, global_id, filter, n_queries, masked, brute), queries, static_cast<xpbd_distance_hit *>(hits_v)};
    with_group_shape(t, n_queries, [&](auto l, auto v, dim3 blocks) {
        hipLaunchKernelGGL((k_distance_pass<decltype(l)::value, decltype(v)::value>), blocks, dim3(64), 0, stream, b, t, a);
    });
    return hipGetLastError();
}

} // namespace xpbd
