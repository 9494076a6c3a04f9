// xpbd_shape_tables.hpp -- the shape tables every kernel reads, compiled on the host from what the caller hands to
// xpbd_world_set_shapes / xpbd_world_set_polytopes (and the multi-GPU world, once for all its shards).  Host-only: no HIP
// header, builds with plain g++ (as xpbd_population_remap.hpp); tests/test_shape_tables_standalone.py holds it to a naive
// restatement.
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/xpbd.h"

namespace xpbd {

constexpr uint32_t kMaxFaceVerts = 8; // vertices per face accepted by the clipper

// Per-shape topology tables in device memory (all shapes back to back).
struct ShapeDesc {
    uint32_t vert0, n_verts;   // into verts (shared with ShapeTable::verts)
    uint32_t face0, n_faces;   // into planes / face_start
    uint32_t edge0, n_edges;   // into edges / edge_dir_id
    uint32_t dir0, n_dirs;     // into edge_dirs: unique edge directions (up to sign)
};

// What the tables' summary says, on the host and on the device (ShapeTables, xpbd_world.hpp) alike.
struct ShapeCounts {
    uint32_t n_shapes = 0, total_verts = 0, max_verts = 0, max_faces = 0, max_face_verts = 0, two_classes = 0, small_max_face_verts = 0;
    bool has_topology = false; // more than the vertex part (verts, vert_offsets, n_shapes, total_verts), which is all compile_vertex_shapes fills
};

// The tables on the host, laid out as PolytopeTables (xpbd_pairs.h) and ShapeTable (xpbd_kernels.h) describe them.
struct ShapeTablesHost : ShapeCounts {
    std::vector<double> verts, planes, centroids, radii, edge_dirs;
    std::vector<uint32_t> vert_offsets, face_start, face_verts, edges, edge_dir_id;
    std::vector<ShapeDesc> desc;
    std::vector<uint8_t> shape_class; // 0: at most 8 vertices and 8 faces, 1: larger
};

// The vertex part from the arguments of xpbd_world_set_shapes, with every check of them that needs no world; refusals name `who`.
int compile_vertex_shapes(const char *who, const double *verts_xyz, const uint32_t *vert_offsets, uint32_t n_shapes, ShapeTablesHost &out);

// All tables from the arguments of xpbd_world_set_polytopes: outward planes (the reference's facing / flip rule), unique edge
// directions up to sign, bounding radii about the centroid, the size class per shape and the maxima the launchers size by.  Its
// own refusals name `who`; those of the vertex part say xpbd_world_set_shapes, which is what checks it.
int compile_polytopes(const char *who, const xpbd_polytope *shapes, uint32_t n_shapes, ShapeTablesHost &out);

} // namespace xpbd
