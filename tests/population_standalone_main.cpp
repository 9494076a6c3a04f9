// population_standalone_main.cpp -- csrc/xpbd_population_remap.cpp built with plain g++ (no hipcc, no ROCm include path; see
// test_population_remap_standalone.py): the joint re-index of a population change against a naive restatement, on 1 000
// random cases of <= 40 bodies and <= 60 joints, and the shared table builders against their definitions.  Exits 0.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../constraint_solver_amd/csrc/xpbd_population_remap.hpp"

namespace {

int failures = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            if (++failures < 20)                                                       \
                std::fprintf(stdout, "line %d: %s (case %u)\n", __LINE__, #cond, g_case); \
        }                                                                              \
    } while (0)

uint32_t g_case = 0;
uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint32_t rnd(uint32_t below) // xorshift64*, below > 0
{
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % below);
}

bool same(const xpbd_joint &a, const xpbd_joint &b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// kind 0: random removal; 1: nobody; 2: everybody
void one_case(uint32_t kind)
{
    const uint32_t n_bodies = 2 + rnd(39), n_joints = rnd(61);
    xpbd::JointSet in;
    for (uint32_t k = 0; k < n_joints; ++k) {
        xpbd_joint j{};
        if (k > 0 && rnd(5) == 0) { // a pair joined twice
            j.body_a = in.joints[k - 1].body_a;
            j.body_b = in.joints[k - 1].body_b;
        } else {
            j.body_a = rnd(n_bodies);
            do
                j.body_b = rnd(n_bodies);
            while (j.body_b == j.body_a); // (both orientations occur: body_a > body_b about half the time)
        }
        j.kind = rnd(3);
        j.distance = (double)k; // a tag that must travel with the joint
        j.anchor_a[0] = 0.25 * k;
        in.joints.push_back(j);
    }
    const uint32_t n_limits = n_joints ? rnd(2 * n_joints) : 0, n_drives = n_joints ? rnd(2 * n_joints) : 0;
    for (uint32_t k = 0; k < n_limits; ++k) {
        xpbd_joint_limit l{};
        l.joint = rnd(n_joints);
        l.kind = rnd(4); // XPBD_LIMIT_* 0..3, SLIDE among them
        l.lower = -(double)k;
        l.upper = (double)k;
        in.limits.push_back(l);
    }
    for (uint32_t k = 0; k < n_drives; ++k) {
        xpbd_joint_drive d{};
        d.joint = rnd(n_joints);
        d.kind = rnd(4);
        d.target = (double)k;
        in.drives.push_back(d);
    }
    std::vector<uint8_t> gone(n_bodies, 0);
    for (uint32_t i = 0; i < n_bodies; ++i)
        gone[i] = kind == 2 || (kind == 0 && rnd(4) == 0);
    std::vector<uint32_t> old_to_new(n_bodies);
    uint32_t n_keep = 0;
    for (uint32_t i = 0; i < n_bodies; ++i)
        old_to_new[i] = gone[i] ? xpbd::kRemoved : n_keep++;

    std::vector<uint32_t> joint_map;
    const xpbd::JointSet out = xpbd::remap_joint_set(in, old_to_new.data(), n_bodies, joint_map);

    // the naive restatement: walk the old joints in order
    CHECK(joint_map.size() == n_joints);
    uint32_t next = 0;
    for (uint32_t k = 0; k < n_joints && joint_map.size() == n_joints; ++k) {
        const xpbd_joint &j = in.joints[k];
        const bool alive = !gone[j.body_a] && !gone[j.body_b];
        if (!alive) {
            CHECK(joint_map[k] == xpbd::kRemoved);
            continue;
        }
        CHECK(joint_map[k] == next); // survivors in order
        if (next < out.joints.size()) {
            xpbd_joint want = j;
            want.body_a = old_to_new[j.body_a];
            want.body_b = old_to_new[j.body_b];
            CHECK(same(out.joints[next], want));
            CHECK((j.body_a > j.body_b) == (out.joints[next].body_a > out.joints[next].body_b)); // orientation kept
            CHECK(out.joints[next].body_a < n_keep && out.joints[next].body_b < n_keep);
        }
        ++next;
    }
    CHECK(out.joints.size() == next);
    // limits and drives follow their joint and keep the caller's order
    size_t at = 0;
    for (const xpbd_joint_limit &l : in.limits) {
        if (joint_map[l.joint] == xpbd::kRemoved)
            continue;
        if (at < out.limits.size()) {
            xpbd_joint_limit want = l;
            want.joint = joint_map[l.joint];
            CHECK(std::memcmp(&out.limits[at], &want, sizeof want) == 0);
        }
        ++at;
    }
    CHECK(out.limits.size() == at);
    at = 0;
    for (const xpbd_joint_drive &d : in.drives) {
        if (joint_map[d.joint] == xpbd::kRemoved)
            continue;
        if (at < out.drives.size()) {
            xpbd_joint_drive want = d;
            want.joint = joint_map[d.joint];
            CHECK(std::memcmp(&out.drives[at], &want, sizeof want) == 0);
        }
        ++at;
    }
    CHECK(out.drives.size() == at);
    if (kind == 1) { // removing nobody is the identity
        CHECK(out.joints.size() == n_joints && out.limits.size() == n_limits && out.drives.size() == n_drives);
        for (uint32_t k = 0; k < n_joints; ++k)
            CHECK(joint_map[k] == k && same(out.joints[k], in.joints[k]));
        CHECK(n_limits == 0 || std::memcmp(out.limits.data(), in.limits.data(), n_limits * sizeof(xpbd_joint_limit)) == 0);
        CHECK(n_drives == 0 || std::memcmp(out.drives.data(), in.drives.data(), n_drives * sizeof(xpbd_joint_drive)) == 0);
    }
    if (kind == 2) // removing everybody leaves nothing
        CHECK(out.joints.empty() && out.limits.empty() && out.drives.empty());

    // the table builders on the result: the CSR lists every joint once per end, ascending inside a body's list
    const xpbd::JointCsr csr = xpbd::build_joint_csr(out.joints.data(), (uint32_t)out.joints.size(), n_keep);
    CHECK(csr.off.size() == (size_t)n_keep + 2 && csr.list.size() == 2 * out.joints.size());
    CHECK(csr.off[0] == 0 && csr.off[n_keep] == 2 * out.joints.size());
    for (uint32_t i = 0; i < n_keep; ++i) {
        CHECK(csr.off[i] <= csr.off[i + 1]);
        for (uint32_t e = csr.off[i]; e < csr.off[i + 1] && e < csr.list.size(); ++e) {
            const uint32_t k = csr.list[e];
            CHECK(k < out.joints.size() && (out.joints[k].body_a == i || out.joints[k].body_b == i));
            CHECK(e == csr.off[i] || csr.list[e - 1] < k);
        }
    }
    // the limit tables: SLIDE limits apart and in order, the angular ones grouped by joint in the caller's order
    const xpbd::LimitTables lt = xpbd::build_limit_tables(out.limits.data(), (uint32_t)out.limits.size(), (uint32_t)out.joints.size());
    CHECK(lt.slide.size() + lt.sorted.size() == out.limits.size() && lt.off.size() == out.joints.size() + 1);
    for (const xpbd_joint_limit &l : lt.slide)
        CHECK(l.kind == XPBD_LIMIT_SLIDE);
    for (uint32_t j = 0; j + 1 < lt.off.size(); ++j) {
        double last = -1.0;
        for (uint32_t e = lt.off[j]; e < lt.off[j + 1] && e < lt.sorted.size(); ++e) {
            CHECK(lt.sorted[e].joint == j && lt.sorted[e].kind != XPBD_LIMIT_SLIDE);
            CHECK(lt.sorted[e].upper > last); // the tags ascend with the caller's order
            last = lt.sorted[e].upper;
        }
    }
    // the extras table: the listed joints ascend, every entry sits under its joint, the slots name the joint in the CSR
    const xpbd::ExtraTables et = xpbd::build_extra_tables(out.joints, lt.slide, out.drives, n_keep);
    if (!et.list.empty()) {
        CHECK(et.off.size() == et.list.size() + 1 && et.slots.size() == 2 * et.list.size());
        CHECK(et.off.back() == lt.slide.size() + out.drives.size() && et.items.size() >= et.off.back() && !et.items.empty());
        for (size_t t = 0; t < et.list.size(); ++t) {
            const uint32_t j = et.list[t];
            CHECK(t == 0 || et.list[t - 1] < j);
            CHECK(j < out.joints.size());
            if (j >= out.joints.size())
                continue;
            CHECK(et.slots[2 * t] < csr.list.size() && csr.list[et.slots[2 * t]] == j);
            CHECK(et.slots[2 * t + 1] < csr.list.size() && csr.list[et.slots[2 * t + 1]] == j);
            CHECK(et.slots[2 * t] >= csr.off[out.joints[j].body_a] && et.slots[2 * t] < csr.off[out.joints[j].body_a + 1]);
            CHECK(et.slots[2 * t + 1] >= csr.off[out.joints[j].body_b] && et.slots[2 * t + 1] < csr.off[out.joints[j].body_b + 1]);
            bool drives_started = false;
            for (uint32_t e = et.off[t]; e < et.off[t + 1]; ++e) {
                CHECK(et.items[e].joint == j);
                const bool is_limit = et.items[e].kind == xpbd::kExtraItemSlideLimit;
                CHECK(!(is_limit && drives_started)); // a joint's SLIDE limits come before its drives
                drives_started = drives_started || !is_limit;
            }
        }
    } else {
        CHECK(lt.slide.empty() && out.drives.empty());
        for (const xpbd_joint &j : out.joints)
            CHECK(j.kind != XPBD_JOINT_SLIDER);
    }
}

} // namespace

int main()
{
    for (g_case = 0; g_case < 1000; ++g_case)
        one_case(g_case % 10 == 8 ? 1u : (g_case % 10 == 9 ? 2u : 0u));
    if (failures) {
        std::fprintf(stdout, "%d checks failed\n", failures);
        return 1;
    }
    std::fprintf(stdout, "population remap: 1000 cases ok\n");
    return 0;
}
