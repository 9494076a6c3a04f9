// xpbd_multi_edit.cpp -- body edits of the multi-GPU world (xpbd_multi.hpp; include/xpbd.h, "Body EDITS"): an edit reaches every
// local shard that HOLDS the body, as owner or as ghost (slot_in_shard over the shard's local_ids).  A shard that fails has not
// done what the others did: shards_disagree.
#include <vector>

#include "xpbd_multi.hpp"

using namespace xpbd::multi;

extern "C" {

int xpbd_multi_world_set_external_wrench(xpbd_multi_world *mw, const uint32_t *indices, uint32_t n, const double *force_xyz,
                                         const double *torque_xyz)
try {
    const char *who = "xpbd_multi_world_set_external_wrench";
    XPBD_TRY(check_usable(mw, who));
    if (n == 0)
        return XPBD_OK;
    if (!force_xyz && !torque_xyz)
        return set_error(XPBD_E_INVALID, "%s: force_xyz and torque_xyz are both NULL", who);
    if (!mw->plan.planned)
        return set_error(XPBD_E_INVALID, "%s: no bodies uploaded", who);
    XPBD_TRY(xpbd::check_edit_indices(who, indices, n, mw->n_global, true));
    XPBD_TRY(xpbd::check_edit_finite(who, "force_xyz", force_xyz, (size_t)n * 3));
    XPBD_TRY(xpbd::check_edit_finite(who, "torque_xyz", torque_xyz, (size_t)n * 3));
    std::vector<uint32_t> slots;
    std::vector<double> force, torque;
    for (Shard &s : mw->shards) {
        slots.clear(), force.clear(), torque.clear();
        for (uint32_t k = 0; k < n; ++k) {
            const int32_t slot = slot_in_shard(s.local_ids, indices ? indices[k] : k);
            if (slot < 0)
                continue;
            slots.push_back((uint32_t)slot);
            if (force_xyz)
                force.insert(force.end(), force_xyz + 3 * (size_t)k, force_xyz + 3 * (size_t)k + 3);
            if (torque_xyz)
                torque.insert(torque.end(), torque_xyz + 3 * (size_t)k, torque_xyz + 3 * (size_t)k + 3);
        }
        if (slots.empty())
            continue;
        if (int rc = xpbd_world_set_external_wrench(s.world, slots.data(), (uint32_t)slots.size(), force_xyz ? force.data() : nullptr,
                                                    torque_xyz ? torque.data() : nullptr))
            return shards_disagree(mw, rc, "external forces");
    }
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

int xpbd_multi_world_apply_impulses(xpbd_multi_world *mw, const xpbd_impulse *list, uint32_t n)
try {
    const char *who = "xpbd_multi_world_apply_impulses";
    XPBD_TRY(check_usable(mw, who));
    if (n == 0)
        return XPBD_OK;
    if (!mw->plan.planned)
        return set_error(XPBD_E_INVALID, "%s: no bodies uploaded", who);
    XPBD_TRY(xpbd::check_impulses(who, list, n, mw->n_global));
    std::vector<xpbd_impulse> local;
    for (Shard &s : mw->shards) {
        local.clear();
        for (uint32_t k = 0; k < n; ++k) { // list order kept: the shard's world sorts by slot (stable), which ascends with the global id
            const int32_t slot = slot_in_shard(s.local_ids, list[k].body);
            if (slot < 0)
                continue;
            local.push_back(list[k]);
            local.back().body = (uint32_t)slot;
        }
        if (local.empty())
            continue;
        if (int rc = xpbd_world_apply_impulses(s.world, local.data(), (uint32_t)local.size()))
            return shards_disagree(mw, rc, "velocities");
    }
    return XPBD_OK;
} XPBD_MULTI_ABI_CATCH

} // extern "C"
