// xpbd_world_shapes.cpp -- the shape tables of the single-GPU world (ShapeTables, xpbd_world.hpp): xpbd_world_set_shapes and
// xpbd_world_set_polytopes.  Both compile on the host (xpbd_shape_tables.hpp), stage every table aside and move the whole set in
// once nothing can fail any more, so a failed call leaves the previous tables in force (one exception: install_shape_tables).
#include <utility>

#include "xpbd_world.hpp"

namespace {

// Every table of `t` in a block of `fresh`, which is allocated unless it is there and large enough; nothing but this allocates or
// copies one.  The device is bound.
int stage_shape_tables(const xpbd::ShapeTablesHost &t, ShapeTables &fresh)
{
    XPBD_TRY(stage_upload(fresh.verts, t.verts.data(), t.verts.size() * 8));
    XPBD_TRY(stage_upload(fresh.vert_offsets, t.vert_offsets.data(), t.vert_offsets.size() * 4));
    static_cast<xpbd::ShapeCounts &>(fresh) = t;
    if (!t.has_topology)
        return XPBD_OK;
    XPBD_TRY(stage_upload(fresh.planes, t.planes.data(), t.planes.size() * 8));
    XPBD_TRY(stage_upload(fresh.centroids, t.centroids.data(), t.centroids.size() * 8));
    XPBD_TRY(stage_upload(fresh.desc, t.desc.data(), t.desc.size() * sizeof(xpbd::ShapeDesc)));
    XPBD_TRY(stage_upload(fresh.face_start, t.face_start.data(), t.face_start.size() * 4));
    XPBD_TRY(stage_upload(fresh.face_verts, t.face_verts.data(), t.face_verts.size() * 4));
    XPBD_TRY(stage_upload(fresh.edges, t.edges.data(), t.edges.size() * 4));
    XPBD_TRY(stage_upload(fresh.radii, t.radii.data(), t.radii.size() * 8));
    XPBD_TRY(stage_upload(fresh.edge_dirs, t.edge_dirs.data(), t.edge_dirs.size() * 8));
    XPBD_TRY(stage_upload(fresh.edge_dir_id, t.edge_dir_id.data(), t.edge_dir_id.size() * 4));
    return stage_upload(fresh.shape_class, t.shape_class.data(), t.shape_class.size());
}

} // namespace

// Compiled tables become the world's (both setters, and every shard of the multi-GPU world from one compilation).  Queued work
// may still read the present tables: the stream is waited for first.
int xpbd::install_shape_tables(xpbd_world *w, const xpbd::ShapeTablesHost &t)
{
    // the resident bodies keep their shape ids: the kernels index the staged table with them unchecked
    if (w->n && t.n_shapes <= w->max_shape_id)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_shapes: %u shapes, but the uploaded bodies use shape id %u (upload bodies "
                                         "again after shrinking the table)", t.n_shapes, w->max_shape_id);
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    ShapeTables fresh;
    // Vertices alone that fit the present blocks are filled into them: xpbd_step_one sets its one shape at every call, and two
    // hipMalloc + two hipFree were 10-20 us of its 80 ("Shape tables").  The world is without shapes meanwhile -- both
    // parts absent, the topology blocks released -- so a failed copy leaves that, not new vertices under old counts.
    ShapeTables &g = w->geom;
    if (!t.has_topology && g.verts.bytes >= at_least_one(t.verts.size()) * 8 && g.vert_offsets.bytes >= t.vert_offsets.size() * 4) {
        fresh.verts = std::move(g.verts);
        fresh.vert_offsets = std::move(g.vert_offsets);
        g.clear();
    }
    XPBD_TRY(stage_shape_tables(t, fresh));
    w->geom = std::move(fresh); // (the previous blocks, stale topology included, go with `fresh`)
    if (t.has_topology)
        w->sleep.wake_all(true);
    return XPBD_OK;
}

extern "C" {

int xpbd_world_set_shapes(xpbd_world *w, const double *verts_xyz, const uint32_t *vert_offsets, uint32_t n_shapes)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_shapes: NULL argument or no shapes");
    xpbd::ShapeTablesHost t;
    XPBD_TRY(xpbd::compile_vertex_shapes("xpbd_world_set_shapes", verts_xyz, vert_offsets, n_shapes, t));
    return xpbd::install_shape_tables(w, t);
} XPBD_ABI_CATCH

int xpbd_world_set_polytopes(xpbd_world *w, const xpbd_polytope *shapes, uint32_t n_shapes)
try {
    if (!w)
        return set_error(XPBD_E_INVALID, "xpbd_world_set_polytopes: NULL argument or no shapes");
    xpbd::ShapeTablesHost t;
    XPBD_TRY(xpbd::compile_polytopes("xpbd_world_set_polytopes", shapes, n_shapes, t));
    return xpbd::install_shape_tables(w, t);
} XPBD_ABI_CATCH

} // extern "C"
