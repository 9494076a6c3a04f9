// xpbd_population_remap.hpp -- what a change of the body population does to the joints (include/xpbd.h, "Body POPULATION"),
// and the host-built tables of the three joint setters.  Host-only: no HIP header, builds with plain g++ (as xpbd_plan.hpp).
#pragma once

#include <cstdint>
#include <vector>

#include "../../include/xpbd.h"

namespace xpbd {

constexpr uint32_t kRemoved = 0xFFFFFFFFu; // XPBD_NO_HIT: what a removed body or a dropped joint maps to

// The joints, limits (all kinds), drives and dampers of a world, as the caller handed them to the four setters.
struct JointSet {
    std::vector<xpbd_joint> joints;
    std::vector<xpbd_joint_limit> limits;
    std::vector<xpbd_joint_drive> drives;
    std::vector<xpbd_joint_damping> damping; // (last: the aggregate initialisers of three vectors stay valid)
};

// The joint set after the bodies were re-indexed by old_to_new ([n_bodies]; kRemoved: the body is gone).  A joint whose two ends
// both survive stays with body_a / body_b re-indexed (a joint given with body_a > body_b keeps that orientation: the map is
// monotone); a joint with a removed end is dropped with its limits, drives and damper.  Surviving joints, limits, drives and
// dampers keep their relative order and name the new joint numbers.  joint_old_to_new: [joints.size()], kRemoved for a dropped one.
JointSet remap_joint_set(const JointSet &in, const uint32_t *old_to_new, uint32_t n_bodies, std::vector<uint32_t> &joint_old_to_new);

// The kinematic table (include/xpbd.h, "KINEMATIC bodies") after the same re-index: the entries of surviving bodies with their
// new body numbers, in order (the map is monotone, so the table stays ascending); those of removed bodies are dropped.
std::vector<xpbd_kinematic> remap_kinematics(const std::vector<xpbd_kinematic> &in, const uint32_t *old_to_new, uint32_t n_bodies);

// CSR body -> joints of xpbd_world_set_joints: off[n_bodies + 1] (allocated n_bodies + 2), list[2 * n_joints] with ascending
// joint index inside every body's list.
struct JointCsr {
    std::vector<uint32_t> off, list;
};
JointCsr build_joint_csr(const xpbd_joint *joints, uint32_t n_joints, uint32_t n_bodies);

// The tables of xpbd_world_set_joint_limits: the SLIDE limits apart (entries of the extras table), the angular ones sorted by
// joint (the caller's order inside a joint) behind a CSR joint -> limits.
struct LimitTables {
    std::vector<xpbd_joint_limit> slide, sorted;
    std::vector<uint32_t> off; // [n_joints + 1]
};
LimitTables build_limit_tables(const xpbd_joint_limit *limits, uint32_t n_limits, uint32_t n_joints);

// One entry of the extras table (mirrors xpbd::JointExtraItem and xpbd_joint_drive: 80 bytes).
constexpr uint32_t kExtraItemSlideLimit = 0x100u; // xpbd::kExtraSlideLimit (xpbd_contacts.h; xpbd_world.cpp asserts it)
struct ExtraItem {
    uint32_t joint, kind;
    double ref_a[3], ref_b[3];
    double target, compliance, max_force;
};
static_assert(sizeof(ExtraItem) == 80 && sizeof(ExtraItem) == sizeof(xpbd_joint_drive), "ExtraItem mirrors xpbd_joint_drive");

// The table k_joint_extras walks: the joints that have extra entries (sliders, SLIDE limits, drives; ascending), where their
// two ends sit in the bodies' joint lists (the CSR above), and per joint its SLIDE limit followed by its drives in the
// caller's order.  list.empty(): no extras.  drive_item: per drive, in the caller's order, its index in `items` (what
// xpbd_world_set_drive_targets edits in place).
struct ExtraTables {
    std::vector<uint32_t> list, slots, off;
    std::vector<ExtraItem> items; // at least one element when !list.empty()
    std::vector<uint32_t> drive_item; // [drives.size()]
};
ExtraTables build_extra_tables(const std::vector<xpbd_joint> &joints, const std::vector<xpbd_joint_limit> &slide_limits,
                               const std::vector<xpbd_joint_drive> &drives, uint32_t n_bodies);

// The table of xpbd_world_set_joint_damping as stage 7 reads it: (mu_l, mu_a) of every joint, zeros for a joint that is not
// listed.  Empty when no entry has a nonzero coefficient: the pass is then off.
std::vector<double> build_joint_damping_table(const std::vector<xpbd_joint_damping> &list, uint32_t n_joints);

} // namespace xpbd
