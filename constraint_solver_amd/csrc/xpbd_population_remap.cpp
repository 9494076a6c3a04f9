// xpbd_population_remap.cpp -- host-only (no HIP header): the joint re-index of a population change and the host-built joint
// tables the three joint setters share with it.
#include <algorithm>
#include <cstring>

#include "xpbd_population_remap.hpp"

namespace xpbd {

JointSet remap_joint_set(const JointSet &in, const uint32_t *old_to_new, uint32_t n_bodies, std::vector<uint32_t> &joint_old_to_new)
{
    JointSet out;
    joint_old_to_new.assign(in.joints.size(), kRemoved);
    for (size_t k = 0; k < in.joints.size(); ++k) {
        const xpbd_joint &j = in.joints[k];
        if (j.body_a >= n_bodies || j.body_b >= n_bodies)
            continue; // (the setters never accept such a joint)
        const uint32_t a = old_to_new[j.body_a], b = old_to_new[j.body_b];
        if (a == kRemoved || b == kRemoved)
            continue;
        joint_old_to_new[k] = (uint32_t)out.joints.size();
        out.joints.push_back(j);
        out.joints.back().body_a = a;
        out.joints.back().body_b = b;
    }
    for (const xpbd_joint_limit &l : in.limits)
        if (l.joint < joint_old_to_new.size() && joint_old_to_new[l.joint] != kRemoved) {
            out.limits.push_back(l);
            out.limits.back().joint = joint_old_to_new[l.joint];
        }
    for (const xpbd_joint_drive &d : in.drives)
        if (d.joint < joint_old_to_new.size() && joint_old_to_new[d.joint] != kRemoved) {
            out.drives.push_back(d);
            out.drives.back().joint = joint_old_to_new[d.joint];
        }
    for (const xpbd_joint_damping &d : in.damping)
        if (d.joint < joint_old_to_new.size() && joint_old_to_new[d.joint] != kRemoved) {
            out.damping.push_back(d);
            out.damping.back().joint = joint_old_to_new[d.joint];
        }
    return out;
}

std::vector<xpbd_kinematic> remap_kinematics(const std::vector<xpbd_kinematic> &in, const uint32_t *old_to_new, uint32_t n_bodies)
{
    std::vector<xpbd_kinematic> out;
    for (const xpbd_kinematic &e : in) {
        if (e.body >= n_bodies || old_to_new[e.body] == kRemoved)
            continue;
        out.push_back(e);
        out.back().body = old_to_new[e.body];
    }
    return out;
}

JointCsr build_joint_csr(const xpbd_joint *joints, uint32_t n_joints, uint32_t n_bodies)
{
    JointCsr c;
    c.off.assign((size_t)n_bodies + 2, 0);
    c.list.resize((size_t)2 * n_joints);
    for (uint32_t k = 0; k < n_joints; ++k) {
        ++c.off[joints[k].body_a + 1];
        ++c.off[joints[k].body_b + 1];
    }
    for (uint32_t i = 0; i < n_bodies; ++i)
        c.off[i + 1] += c.off[i];
    std::vector<uint32_t> cursor(c.off.begin(), c.off.end() - 1);
    for (uint32_t k = 0; k < n_joints; ++k) { // ascending joint index inside every body's list
        c.list[cursor[joints[k].body_a]++] = k;
        c.list[cursor[joints[k].body_b]++] = k;
    }
    return c;
}

LimitTables build_limit_tables(const xpbd_joint_limit *limits, uint32_t n_limits, uint32_t n_joints)
{
    LimitTables t;
    // the SLIDE limits are entries of k_joint_extras, not of the pair solve's table
    for (uint32_t k = 0; k < n_limits; ++k)
        if (limits[k].kind == XPBD_LIMIT_SLIDE)
            t.slide.push_back(limits[k]);
    // CSR joint -> angular limits, the caller's order inside a joint
    t.off.assign((size_t)n_joints + 1, 0);
    for (uint32_t k = 0; k < n_limits; ++k)
        if (limits[k].kind != XPBD_LIMIT_SLIDE)
            ++t.off[limits[k].joint + 1];
    for (uint32_t j = 0; j < n_joints; ++j)
        t.off[j + 1] += t.off[j];
    t.sorted.resize(n_limits - t.slide.size());
    std::vector<uint32_t> cursor(t.off.begin(), t.off.end() - 1);
    for (uint32_t k = 0; k < n_limits; ++k)
        if (limits[k].kind != XPBD_LIMIT_SLIDE)
            t.sorted[cursor[limits[k].joint]++] = limits[k];
    return t;
}

ExtraTables build_extra_tables(const std::vector<xpbd_joint> &joints, const std::vector<xpbd_joint_limit> &slide_limits,
                               const std::vector<xpbd_joint_drive> &drives, uint32_t n_bodies)
{
    ExtraTables t;
    const uint32_t n = (uint32_t)joints.size();
    std::vector<uint32_t> count(n, 0);
    std::vector<uint8_t> listed(n, 0);
    for (uint32_t j = 0; j < n; ++j)
        listed[j] = joints[j].kind == XPBD_JOINT_SLIDER;
    for (const xpbd_joint_limit &l : slide_limits)
        ++count[l.joint], listed[l.joint] = 1;
    for (const xpbd_joint_drive &d : drives)
        ++count[d.joint], listed[d.joint] = 1;
    std::vector<uint32_t> first(n, 0);
    t.off.assign(1, 0);
    for (uint32_t j = 0; j < n; ++j)
        if (listed[j]) {
            t.list.push_back(j);
            first[j] = t.off.back();
            t.off.push_back(t.off.back() + count[j]);
        }
    if (t.list.empty())
        return t;
    // where the two ends of a listed joint sit in the bodies' joint lists (the CSR of xpbd_world_set_joints)
    std::vector<uint32_t> slot_cursor((size_t)n_bodies + 1, 0);
    t.slots.resize(2 * t.list.size());
    for (const xpbd_joint &j : joints) {
        ++slot_cursor[j.body_a + 1];
        ++slot_cursor[j.body_b + 1];
    }
    for (uint32_t i = 0; i < n_bodies; ++i)
        slot_cursor[i + 1] += slot_cursor[i];
    for (uint32_t j = 0, k = 0; j < n; ++j) {
        const uint32_t slot_a = slot_cursor[joints[j].body_a]++, slot_b = slot_cursor[joints[j].body_b]++;
        if (listed[j]) {
            t.slots[2 * k] = slot_a, t.slots[2 * k + 1] = slot_b;
            ++k;
        }
    }
    t.items.assign(std::max<size_t>(t.off.back(), 1), ExtraItem{});
    std::vector<uint32_t> cursor = first;
    for (const xpbd_joint_limit &l : slide_limits) {
        ExtraItem it{};
        it.joint = l.joint, it.kind = kExtraItemSlideLimit, it.target = l.lower, it.compliance = l.upper;
        t.items[cursor[l.joint]++] = it;
    }
    t.drive_item.reserve(drives.size());
    for (const xpbd_joint_drive &d : drives) {
        t.drive_item.push_back(cursor[d.joint]);
        std::memcpy(&t.items[cursor[d.joint]++], &d, sizeof d);
    }
    return t;
}

std::vector<double> build_joint_damping_table(const std::vector<xpbd_joint_damping> &list, uint32_t n_joints)
{
    bool any = false;
    for (const xpbd_joint_damping &d : list)
        any = any || (d.joint < n_joints && (d.linear != 0.0 || d.angular != 0.0));
    std::vector<double> table;
    if (!any)
        return table;
    table.assign((size_t)2 * n_joints, 0.0);
    for (const xpbd_joint_damping &d : list)
        if (d.joint < n_joints) {
            table[(size_t)2 * d.joint] = d.linear;
            table[(size_t)2 * d.joint + 1] = d.angular;
        }
    return table;
}

} // namespace xpbd
