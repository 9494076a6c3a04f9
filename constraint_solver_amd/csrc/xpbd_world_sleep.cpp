// xpbd_world_sleep.cpp -- island sleeping of the single-GPU world: Sleep (xpbd_world.hpp) and the sleeping entry points.
// Semantics: include/xpbd.h, "SLEEPING"; the kernels: xpbd_sleep.hip.
#include <cmath>

#include "xpbd_world.hpp"

namespace {

xpbd::SleepTarget sleep_target(const xpbd_world *w)
{
    return xpbd::SleepTarget{w->mode, w->n, w->report.on, w->sleep.on};
}

} // namespace

// Room for the world's stride; a fresh state starts every body awake with zero counters.  Queued work may still use the
// blocks: the stream is waited for only when one has to grow (a new stride: the state is fresh then anyway).
int Sleep::ensure(const xpbd_world *w)
{
    const size_t st = w->stride ? w->stride : 256u;
    XPBD_HIP_TRY(xpbd::reserve_after_sync(w->stream, {{state, state_bytes((uint32_t)st)}, {scratch, st * 7}}));
    if (fresh) {
        XPBD_HIP_TRY(hipMemsetAsync(state.ptr, 0, state_bytes((uint32_t)st), w->stream));
        XPBD_HIP_TRY(hipMemsetAsync(state.as<uint32_t>() + st, 0xFF, st * 4, w->stream)); // group = XPBD_SLEEP_GROUP_NONE
        fresh = false;
    }
    return XPBD_OK;
}

int Sleep::frame_begin(xpbd_world *w)
{
    XPBD_TRY(ensure(w));
    XPBD_HIP_TRY(xpbd::launch_sleep_frame_begin(view(w), w->stat.as<double>(), requests, w->stream));
    if (moving) // a MOVING kinematic body is not inert in this frame ("KINEMATIC bodies"; no table: the launches of before)
        XPBD_HIP_TRY(xpbd::launch_sleep_moving_inert(view(w), w->kinematics.view(), w->stream));
    XPBD_TRY(sensor_not_inert(w)); // a sensor is never inert ("SENSOR bodies"; no sensor: nothing)
    requests = 0;
    return XPBD_OK;
}

int Sleep::frame_records(xpbd_world *w, uint32_t *trace, uint32_t trace_rows)
{
    XPBD_HIP_TRY(xpbd::launch_sleep_records(view(w), w->arrays(), w->cb_rec.as<double>(), w->cb_rec_b.as<double>(),
                                            w->restitution.on ? w->dyn_alt.as<double>() : nullptr, w->last_mask.as<uint32_t>(), trace, trace_rows,
                                            w->stream));
    return XPBD_OK;
}

// The sleep pass, enqueued only.  The touching pairs are the report's keys of the frame, compacted now if they are not (as
// Islands::enqueue does); the grouping is the islands unit's own.
int Sleep::frame_end(xpbd_world *w)
{
    const xpbd::SleepState s = view(w);
    const unsigned long long *keys = nullptr;
    const uint32_t *key_count = nullptr;
    if (w->bp.n_pairs)
        XPBD_TRY(contact_edge_keys(w, &keys, &key_count)); // (without the sensor pairs: "SENSOR bodies")
    xpbd::MovingBodies mv; // the frame's MOVING kinematic bodies mark what shares a pair of the pair list or a joint with them
    if (moving)
        mv = xpbd::MovingBodies{s.moving, w->bp.pairs.as<uint32_t>(), w->bp.n_pairs, w->joints.csr.joints.as<xpbd::Joint>(), w->joints.csr.n};
    XPBD_HIP_TRY(xpbd::launch_sleep_wake_count(s, w->dyn.as<double>(), keys, key_count, w->bp.n_pairs, cfg.linear_speed * cfg.linear_speed,
                                               cfg.angular_speed * cfg.angular_speed, w->stream, mv));
    Islands &isl = w->islands;
    XPBD_TRY(isl.reserve(w, false, 0));
    uint32_t *result = isl.result.as<uint32_t>();
    XPBD_TRY(isl.enqueue(w, 0, nullptr, nullptr, 0, result + 1));
    XPBD_HIP_TRY(xpbd::launch_sleep_islands(s, w->dyn.as<double>(), isl.parent.as<uint32_t>(), result, cfg.frames_to_sleep, w->stream));
    return XPBD_OK;
}

int Sleep::request(xpbd_world *w, const uint32_t *dev_indices, uint32_t every, uint32_t n)
{
    XPBD_TRY(ensure(w));
    XPBD_HIP_TRY(xpbd::launch_sleep_request(view(w), w->stat.as<double>(), dev_indices, every, n, w->stream));
    return XPBD_OK;
}

int Sleep::request_drives(xpbd_world *w, const uint32_t *dev_drives, const double *dev_targets, uint32_t n)
{
    XPBD_TRY(ensure(w));
    XPBD_HIP_TRY(xpbd::launch_sleep_request_drives(view(w), w->joints.drive_table(), w->joints.csr.joints.as<xpbd::Joint>(), w->joints.csr.n, dev_drives,
                                                   dev_targets, n, w->stream));
    return XPBD_OK;
}

extern "C" {

int xpbd_world_set_sleeping(xpbd_world *w, const xpbd_sleep_config *cfg)
try {
    static_assert(sizeof(xpbd_sleep_config) == 24, "xpbd_sleep_config is {linear_speed, angular_speed, frames_to_sleep, flags}");
    const char *who = "xpbd_world_set_sleeping";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    if (cfg)
        XPBD_TRY(sleep_target(w).check(who, *cfg));
    Sleep &s = w->sleep;
    if ((cfg != nullptr) != s.on) { // the size of a history entry changes: the entries go
        w->history.length = 0;
        w->history.stepped.clear();
        w->history.sleep_requests.clear();
        s.fresh = true;
        s.requests = 0;
        w->bp.have_neighbours = false; // (a pair list made under the other rule)
    }
    s.on = cfg != nullptr;
    if (cfg)
        s.cfg = *cfg;
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_sleep_state(xpbd_world *w, uint8_t *asleep, uint32_t *rest_frames, uint32_t *group, uint32_t counts[4])
try {
    const char *who = "xpbd_world_sleep_state";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    XPBD_TRY(sleep_target(w).state_check(who));
    XPBD_TRY(bind_device(w));
    XPBD_TRY(w->sleep.ensure(w));
    const xpbd::SleepState s = w->sleep.view(w);
    uint32_t ctrl[5] = {0, 0, 0, 0, 0};
    if (counts) {
        XPBD_HIP_TRY(xpbd::launch_sleep_tally(s, w->stream));
        XPBD_HIP_TRY(hipMemcpyAsync(ctrl, s.ctrl, sizeof ctrl, hipMemcpyDeviceToHost, w->stream));
    }
    if (asleep && w->n)
        XPBD_HIP_TRY(hipMemcpyAsync(asleep, s.asleep, w->n, hipMemcpyDeviceToHost, w->stream));
    if (rest_frames && w->n)
        XPBD_HIP_TRY(hipMemcpyAsync(rest_frames, s.rest_frames, (size_t)w->n * 4, hipMemcpyDeviceToHost, w->stream));
    if (group && w->n)
        XPBD_HIP_TRY(hipMemcpyAsync(group, s.group, (size_t)w->n * 4, hipMemcpyDeviceToHost, w->stream));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream));
    if (counts) {
        counts[0] = ctrl[xpbd::SC_ASLEEP];
        counts[1] = ctrl[xpbd::SC_GROUPS];
        counts[2] = ctrl[xpbd::SC_WOKEN];
        counts[3] = ctrl[xpbd::SC_SLEPT];
    }
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_sleep_state_device(xpbd_world *w, uint8_t *dev_asleep, uint32_t *dev_rest_frames, uint32_t *dev_group, uint32_t *dev_counts)
try {
    const char *who = "xpbd_world_sleep_state_device";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    XPBD_TRY(sleep_target(w).state_check(who));
    XPBD_TRY(bind_device(w));
    XPBD_TRY(w->sleep.ensure(w));
    const xpbd::SleepState s = w->sleep.view(w);
    if (dev_counts) {
        XPBD_HIP_TRY(xpbd::launch_sleep_tally(s, w->stream));
        XPBD_HIP_TRY(hipMemcpyAsync(dev_counts, s.ctrl + xpbd::SC_ASLEEP, 8, hipMemcpyDeviceToDevice, w->stream));
        XPBD_HIP_TRY(hipMemcpyAsync(dev_counts + 2, s.ctrl + xpbd::SC_WOKEN, 8, hipMemcpyDeviceToDevice, w->stream));
    }
    if (dev_asleep && w->n)
        XPBD_HIP_TRY(hipMemcpyAsync(dev_asleep, s.asleep, w->n, hipMemcpyDeviceToDevice, w->stream));
    if (dev_rest_frames && w->n)
        XPBD_HIP_TRY(hipMemcpyAsync(dev_rest_frames, s.rest_frames, (size_t)w->n * 4, hipMemcpyDeviceToDevice, w->stream));
    if (dev_group && w->n)
        XPBD_HIP_TRY(hipMemcpyAsync(dev_group, s.group, (size_t)w->n * 4, hipMemcpyDeviceToDevice, w->stream));
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_wake_bodies(xpbd_world *w, const uint32_t *indices, uint32_t n)
try {
    const char *who = "xpbd_world_wake_bodies";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    XPBD_TRY(sleep_target(w).wake_check(who, indices, n));
    if (!indices) {
        w->sleep.wake_all(false);
        return XPBD_OK;
    }
    if (n == 0)
        return XPBD_OK;
    XPBD_TRY(bind_device(w));
    XPBD_HIP_TRY(xpbd::reserve_after_sync(w->stream, {{w->edit.indices, (size_t)n * 4}}));
    XPBD_HIP_TRY(hipMemcpyAsync(w->edit.indices.ptr, indices, (size_t)n * 4, hipMemcpyHostToDevice, w->stream));
    XPBD_TRY(w->sleep.request(w, w->edit.indices.as<uint32_t>(), 1, n));
    XPBD_HIP_TRY(hipStreamSynchronize(w->stream)); // the caller's array is only borrowed
    return XPBD_OK;
} XPBD_ABI_CATCH

int xpbd_world_wake_bodies_device(xpbd_world *w, const uint32_t *dev_indices, uint32_t n)
try {
    const char *who = "xpbd_world_wake_bodies_device";
    if (!w)
        return set_error(XPBD_E_INVALID, "%s: NULL world", who);
    XPBD_TRY(sleep_target(w).state_check(who));
    if (!dev_indices && n)
        return set_error(XPBD_E_INVALID, "%s: NULL dev_indices with n = %u (NULL with n == 0 wakes everybody)", who, n);
    if (!dev_indices) {
        w->sleep.wake_all(false);
        return XPBD_OK;
    }
    XPBD_TRY(bind_device(w));
    return w->sleep.request(w, dev_indices, 1, n);
} XPBD_ABI_CATCH

} // extern "C"
