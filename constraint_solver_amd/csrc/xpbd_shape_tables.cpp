// xpbd_shape_tables.cpp -- the shape tables compiled on the host (xpbd_shape_tables.hpp).
// Host-only: no HIP header, builds with plain g++ (as xpbd_population_remap.cpp).  The arithmetic reaches device results that
// tests compare bit for bit: every expression keeps its order, and the unit is compiled with -ffp-contract=off like the rest.
#include "xpbd_shape_tables.hpp"

#include "xpbd_error.h"
#include "xpbd_math.hpp"

namespace xpbd {

int compile_vertex_shapes(const char *who, const double *verts_xyz, const uint32_t *vert_offsets, uint32_t n_shapes, ShapeTablesHost &out)
{
    if (!verts_xyz || !vert_offsets || n_shapes == 0)
        return set_error(XPBD_E_INVALID, "%s: NULL argument or no shapes", who);
    if (vert_offsets[0] != 0)
        return set_error(XPBD_E_INVALID, "%s: vert_offsets[0] must be 0", who);
    for (uint32_t s = 0; s < n_shapes; ++s) {
        if (vert_offsets[s + 1] < vert_offsets[s])
            return set_error(XPBD_E_INVALID, "%s: vert_offsets not monotone at %u", who, s);
        if (vert_offsets[s + 1] - vert_offsets[s] > XPBD_MAX_SHAPE_VERTS)
            return set_error(XPBD_E_INVALID, "%s: shape %u has %u vertices (max %u)", who, s, vert_offsets[s + 1] - vert_offsets[s], XPBD_MAX_SHAPE_VERTS);
    }
    const uint32_t total = vert_offsets[n_shapes];
    // The tables are staged into LDS by every block; keep them far below the 160 KiB/CU.
    if ((size_t)total * 24 + (size_t)(n_shapes + 1) * 4 > 48 * 1024)
        return set_error(XPBD_E_INVALID, "%s: shape tables exceed 48 KiB", who);
    out.verts.assign(verts_xyz, verts_xyz + 3 * (size_t)total);
    out.vert_offsets.assign(vert_offsets, vert_offsets + n_shapes + 1);
    out.n_shapes = n_shapes;
    out.total_verts = total;
    return XPBD_OK;
}

int compile_polytopes(const char *who, const xpbd_polytope *shapes, uint32_t n_shapes, ShapeTablesHost &out)
{
    if (!shapes || n_shapes == 0)
        return set_error(XPBD_E_INVALID, "%s: NULL argument or no shapes", who);
    out = ShapeTablesHost{};
    std::vector<double> verts;
    std::vector<uint32_t> vert_offsets{0};
    out.face_start.push_back(0);
    uint32_t n_small = 0;
    for (uint32_t s = 0; s < n_shapes; ++s) {
        const xpbd_polytope &p = shapes[s];
        if ((p.n_vertices && !p.vertices_xyz) || (p.n_edges && !p.edges) || (p.n_faces && (!p.face_offsets || !p.face_indices)))
            return set_error(XPBD_E_INVALID, "%s: shape %u has a NULL table", who, s);
        if (p.n_vertices > XPBD_MAX_SHAPE_VERTS || p.n_faces > 64 || p.n_edges > 4096)
            return set_error(XPBD_E_INVALID, "%s: shape %u too large (%u vertices, %u faces, %u edges)", who, s, p.n_vertices, p.n_faces, p.n_edges);
        ShapeDesc d{};
        d.vert0 = (uint32_t)(verts.size() / 3);
        d.n_verts = p.n_vertices;
        d.face0 = (uint32_t)(out.planes.size() / 4);
        d.n_faces = p.n_faces;
        d.edge0 = (uint32_t)(out.edges.size() / 2);
        d.n_edges = p.n_edges;
        verts.insert(verts.end(), p.vertices_xyz, p.vertices_xyz + 3 * (size_t)p.n_vertices);
        vert_offsets.push_back((uint32_t)(verts.size() / 3));
        auto vertex = [&](uint32_t i) { return Vec3{p.vertices_xyz[3 * i], p.vertices_xyz[3 * i + 1], p.vertices_xyz[3 * i + 2]}; };
        for (uint32_t e = 0; e < 2 * p.n_edges; ++e) {
            if (p.edges[e] >= p.n_vertices)
                return set_error(XPBD_E_INVALID, "%s: shape %u edge vertex out of range", who, s);
            out.edges.push_back(p.edges[e]);
        }
        // unique edge directions (up to sign), first edge with a direction represents it
        std::vector<double> &dirs = out.edge_dirs;
        d.dir0 = (uint32_t)(dirs.size() / 3);
        for (uint32_t e = 0; e < p.n_edges; ++e) {
            const Vec3 dv = vertex(p.edges[2 * e + 1]) - vertex(p.edges[2 * e]);
            const uint32_t nd = (uint32_t)(dirs.size() / 3) - d.dir0;
            uint32_t found = nd;
            for (uint32_t k = 0; k < nd; ++k) {
                const double *u = &dirs[3 * (size_t)(d.dir0 + k)];
                const Vec3 uv{u[0], u[1], u[2]};
                const Vec3 c = cross(dv, uv);
                if (dot(c, c) <= 1e-12 * (dot(dv, dv) * dot(uv, uv))) {
                    found = k;
                    break;
                }
            }
            if (found == nd)
                dirs.insert(dirs.end(), {dv.x, dv.y, dv.z});
            out.edge_dir_id.push_back(found);
        }
        d.n_dirs = (uint32_t)(dirs.size() / 3) - d.dir0;
        const Vec3 centroid{p.centroid[0], p.centroid[1], p.centroid[2]};
        const bool small = p.n_vertices <= 8 && p.n_faces <= 8;
        for (uint32_t f = 0; f < p.n_faces; ++f) {
            const uint32_t f0 = p.face_offsets[f], f1 = p.face_offsets[f + 1];
            if (f1 < f0 || f1 - f0 < 3 || f1 - f0 > kMaxFaceVerts)
                return set_error(XPBD_E_INVALID, "%s: shape %u face %u needs 3..%u vertices", who, s, f, kMaxFaceVerts);
            for (uint32_t q = f0; q < f1; ++q) {
                if (p.face_indices[q] >= p.n_vertices)
                    return set_error(XPBD_E_INVALID, "%s: shape %u face vertex out of range", who, s);
                out.face_verts.push_back(p.face_indices[q]);
            }
            out.face_start.push_back((uint32_t)out.face_verts.size());
            // Polytope::plane (src/geometry.rs:262-271) over Plane::from_points / facing / flip (:16-24, :55-68)
            const Vec3 p0 = vertex(p.face_indices[f0]), p1 = vertex(p.face_indices[f0 + 1]), p2 = vertex(p.face_indices[f0 + 2]);
            Vec3 n = normalized(cross(p1 - p0, p2 - p0));
            double disp = dot(n, p0);
            const bool facing = dot(n, centroid - disp * n) >= 0.0;
            if (facing) {
                n = -n;
                disp = -disp;
            }
            out.planes.insert(out.planes.end(), {n.x, n.y, n.z, disp});
            out.max_face_verts = f1 - f0 > out.max_face_verts ? f1 - f0 : out.max_face_verts;
            if (small)
                out.small_max_face_verts = f1 - f0 > out.small_max_face_verts ? f1 - f0 : out.small_max_face_verts;
        }
        out.centroids.insert(out.centroids.end(), {centroid.x, centroid.y, centroid.z});
        double radius = 0.0; // bounding sphere about the centroid
        for (uint32_t k = 0; k < p.n_vertices; ++k) {
            const double dist = length(vertex(k) - centroid);
            if (dist > radius)
                radius = dist;
        }
        out.radii.push_back(radius);
        out.desc.push_back(d);
        out.max_verts = p.n_vertices > out.max_verts ? p.n_vertices : out.max_verts;
        out.max_faces = p.n_faces > out.max_faces ? p.n_faces : out.max_faces;
        out.shape_class.push_back(small ? 0 : 1);
        n_small += small;
    }
    out.two_classes = (n_small != 0 && n_small != n_shapes) ? 1u : 0u;
    static const double zero3[3] = {0, 0, 0};
    XPBD_TRY(compile_vertex_shapes("xpbd_world_set_shapes", verts.empty() ? zero3 : verts.data(), vert_offsets.data(), n_shapes, out));
    out.has_topology = true;
    return XPBD_OK;
}

} // namespace xpbd
