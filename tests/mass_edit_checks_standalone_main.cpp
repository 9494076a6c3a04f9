// mass_edit_checks_standalone_main.cpp -- MassEditTarget (csrc/xpbd_checks.cpp, declared in csrc/xpbd_checks.hpp), the argument
// checks of xpbd_world_set_mass_properties(_device) and xpbd_world_get_mass_properties, and the row rules they share with the
// kernel (csrc/xpbd_mass_row.hpp), built with plain g++ (no hipcc, no ROCm include path; see
// test_mass_edit_checks_standalone.py): every way the checks refuse a call, each with its code and a message that names the `who`
// it was given and the reason, and the calls they accept.  Exits 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../constraint_solver_amd/csrc/xpbd_checks.hpp"
#include "../constraint_solver_amd/csrc/xpbd_mass_row.hpp"

namespace {

int failures = 0, calls = 0;

void accepted(int rc, const char *what)
{
    ++calls;
    if (rc != XPBD_OK) {
        ++failures;
        std::printf("%s: accepted call returned %d (%s)\n", what, rc, xpbd_last_error());
    }
}

void refused(int rc, const char *who, const char *word, int code = XPBD_E_INVALID)
{
    ++calls;
    if (rc != code || !std::strstr(xpbd_last_error(), who) || !std::strstr(xpbd_last_error(), word)) {
        ++failures;
        std::printf("%s: refused call returned %d with message '%s' (expected %d and '%s' in it)\n", who, rc, xpbd_last_error(), code, word);
    }
}

xpbd_kinematic entry(uint32_t body)
{
    xpbd_kinematic e{};
    e.body = body;
    e.mode = XPBD_KINEMATIC_POSE;
    e.angular[0] = 1.0;
    return e;
}

// n rows: inverse_mass | mass 0.5, the identity, centre of mass (0.1, 0.2, 0.3): valid in both layouts
std::vector<double> rows_of(uint32_t n)
{
    std::vector<double> r((size_t)n * 13, 0.0);
    for (uint32_t k = 0; k < n; ++k) {
        double *row = r.data() + (size_t)k * 13;
        row[0] = 0.5;
        row[1] = row[5] = row[9] = 1.0 + k;
        row[10] = 0.1, row[11] = 0.2, row[12] = 0.3;
    }
    return r;
}

} // namespace

int main()
{
    using namespace xpbd;
    const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
    const std::vector<xpbd_kinematic> table = {entry(2), entry(5)};
    const MassEditTarget world{8, table.data(), 2}, plain{8, nullptr, 0}, empty{0, nullptr, 0};
    const uint32_t some[3] = {6, 0, 3}, twice[3] = {1, 4, 1}, outside[2] = {1, 8}, held[2] = {1, 5}, all[8] = {7, 6, 5, 4, 3, 2, 1, 0};
    const std::vector<double> r3 = rows_of(3), r8 = rows_of(8);
    const uint32_t keep = XPBD_MASS_KEEP_FRAME;

    // ---- the flags ----
    static_assert(XPBD_MASS_INVERSE == 0u && XPBD_MASS_DIRECT == 1u && XPBD_MASS_KEEP_FRAME == 0x100u, "the flags of the header");
    if (!mass_flags_known(0) || !mass_flags_known(1) || !mass_flags_known(keep) || !mass_flags_known(keep | 1u) || mass_flags_known(2) ||
        mass_flags_known(0x200) || mass_flags_known(keep | 3u) || mass_flags_known(0x80000000u))
        ++failures;

    // ---- xpbd_world_set_mass_properties (host) ----
    for (uint32_t flags : {0u, 1u, keep, keep | 1u}) {
        accepted(plain.check("ok_list", some, 3, r3.data(), flags, true), "an unordered subset, every layout and flag");
        accepted(plain.check("ok_all", nullptr, 8, r8.data(), flags, true), "NULL indices with n == the body count");
    }
    accepted(world.check("ok_beside_kinematic", some, 3, r3.data(), XPBD_MASS_INVERSE, true), "mass for bodies that are not in the table");
    {
        std::vector<double> r = rows_of(2);
        for (int c = 0; c < 10; ++c)
            r[13 + c] = c % 2 ? 0.0 : -0.0; // body 5 stays fixed; its centre of mass may change
        accepted(world.check("ok_kinematic_stays_fixed", held, 2, r.data(), XPBD_MASS_INVERSE, true), "a kinematic body keeps zeros");
        accepted(world.check("ok_kinematic_keep_frame", held, 2, r.data(), keep, true), "... also with KEEP_FRAME");
        r[0] = 0.0;
        accepted(plain.check("ok_zero_inverse_mass", held, 2, r.data(), XPBD_MASS_INVERSE, true), "inverse_mass == 0 with inertia");
        r[0] = -0.0;
        accepted(plain.check("ok_minus_zero", held, 2, r.data(), XPBD_MASS_INVERSE, true), "-0.0 is not negative");
        r[13] = 1e-300; // DIRECT: a tiny mass is positive
        r[14] = r[18] = r[22] = 1.0;
        r[0] = 2.0;
        accepted(plain.check("ok_tiny_mass", held, 2, r.data(), XPBD_MASS_DIRECT, true), "a tiny positive mass");
    }
    refused(plain.check("null_rows", some, 3, nullptr, 0, true), "null_rows", "NULL rows");
    refused(empty.check("no_bodies", some, 3, r3.data(), 0, true), "no_bodies", "holds no bodies");
    refused(plain.check("count", nullptr, 3, r3.data(), 0, true), "count", "holds 8 bodies");
    refused(plain.check("range", outside, 2, r3.data(), 0, true), "range", "indices[1] = 8");
    refused(plain.check("twice", twice, 3, r3.data(), 0, true), "twice", "listed twice");
    refused(plain.check("flag_bits", some, 3, r3.data(), 0x200, true), "flag_bits", "unknown flags 0x200");
    refused(plain.check("layout", some, 3, r3.data(), 2, true), "layout", "unknown flags 0x2");
    refused(plain.check("layout_keep", some, 3, r3.data(), keep | 7u, true), "layout_keep", "unknown flags 0x107");
    for (uint32_t flags : {0u, 1u}) {
        for (int c = 0; c < 13; ++c) {
            for (double bad : {nan, inf, -inf}) {
                std::vector<double> r = r3;
                r[13 * (c % 3) + c] = bad;
                refused(plain.check("finite", some, 3, r.data(), flags, true), "finite", "not finite");
            }
        }
    }
    {
        std::vector<double> r = r3;
        r[26] = -1e-300;
        refused(plain.check("negative", some, 3, r.data(), XPBD_MASS_INVERSE, true), "negative", "rows[2] has inverse_mass");
        r = r3;
        r[13] = 0.0;
        refused(plain.check("zero_mass", some, 3, r.data(), XPBD_MASS_DIRECT, true), "zero_mass", "rows[1] has mass = 0");
        r[13] = -3.0;
        refused(plain.check("negative_mass", some, 3, r.data(), XPBD_MASS_DIRECT | keep, true), "negative_mass", "needs mass > 0");
        r = r3; // singular tensors: a zero row, two equal columns, all zeros
        r[2] = r[5] = r[8] = 0.0, r[1] = 2.0, r[3] = 1.0, r[4] = 0.5, r[6] = 3.0, r[7] = 1.0, r[9] = 4.0;
        refused(plain.check("singular_row", some, 3, r.data(), XPBD_MASS_DIRECT, true), "singular_row", "rows[0]: the inertia tensor is not invertible",
                XPBD_E_SINGULAR_INERTIA);
        r = r3;
        for (int c = 0; c < 3; ++c)
            r[14 + c] = r[17 + c] = 1.0 + c;
        refused(plain.check("singular_columns", some, 3, r.data(), XPBD_MASS_DIRECT, true), "singular_columns", "rows[1]", XPBD_E_SINGULAR_INERTIA);
        r = r3;
        for (int c = 1; c < 10; ++c)
            r[26 + c] = 0.0;
        refused(plain.check("singular_zero", some, 3, r.data(), XPBD_MASS_DIRECT | keep, true), "singular_zero", "determinant is 0", XPBD_E_SINGULAR_INERTIA);
        accepted(plain.check("ok_zero_inertia_inverse", some, 3, r.data(), XPBD_MASS_INVERSE, true), "the INVERSE layout takes a zero inverse inertia");
    }
    {
        const std::vector<double> r = rows_of(2); // body 5 has an entry in the table
        refused(world.check("kinematic_mass", held, 2, r.data(), XPBD_MASS_INVERSE, true), "kinematic_mass", "gives mass to body 5");
        refused(world.check("kinematic_direct", held, 2, r.data(), XPBD_MASS_DIRECT, true), "kinematic_direct", "entry in the kinematic table");
        std::vector<double> z = r;
        for (int c = 0; c < 10; ++c)
            z[13 + c] = 0.0;
        z[13 + 9] = 1e-300; // one inertia entry is enough
        refused(world.check("kinematic_inertia", held, 2, z.data(), keep, true), "kinematic_inertia", "gives mass to body 5");
        std::vector<double> r8k = r8; // the NULL form names body 2 too
        refused(world.check("kinematic_all", nullptr, 8, r8k.data(), XPBD_MASS_INVERSE, true), "kinematic_all", "rows[2] gives mass to body 2");
    }

    // ---- xpbd_world_set_mass_properties_device: it reads neither list ----
    std::vector<double> junk(26, nan);
    accepted(world.check("d_ok", outside, 2, junk.data(), XPBD_MASS_DIRECT | keep, false), "the device variant cannot see values or indices");
    accepted(world.check("d_ok_twice", twice, 3, r3.data(), 0, false), "... nor a repeated index");
    accepted(world.check("d_ok_all", nullptr, 8, r8.data(), 1, false), "NULL indices with n == the body count");
    accepted(world.check("d_ok_more", all, (1u << 29), r8.data(), 0, false), "2^29 entries");
    refused(world.check("d_null_rows", some, 3, nullptr, 0, false), "d_null_rows", "NULL rows");
    refused(empty.check("d_no_bodies", some, 3, r3.data(), 0, false), "d_no_bodies", "holds no bodies");
    refused(world.check("d_count", nullptr, 3, r3.data(), 0, false), "d_count", "holds 8 bodies");
    refused(world.check("d_too_many", all, (1u << 29) + 1u, r8.data(), 0, false), "d_too_many", "2^29");
    refused(world.check("d_alignment", some, 3, reinterpret_cast<const double *>(reinterpret_cast<const char *>(r3.data()) + 4), 0, false), "d_alignment",
            "8-byte aligned");
    refused(world.check("d_flag_bits", some, 3, r3.data(), 0x400, false), "d_flag_bits", "unknown flags 0x400");
    refused(world.check("d_layout", some, 3, r3.data(), keep | 2u, false), "d_layout", "unknown flags 0x102");

    // ---- xpbd_world_get_mass_properties ----
    double out[39];
    accepted(plain.get_check("g_ok", some, 3, out), "a subset");
    accepted(plain.get_check("g_ok_twice", twice, 3, out), "an index may repeat in a read");
    accepted(plain.get_check("g_ok_all", nullptr, 8, out), "NULL indices with n == the body count");
    refused(plain.get_check("g_null_rows", some, 3, nullptr), "g_null_rows", "NULL rows");
    refused(empty.get_check("g_no_bodies", some, 3, out), "g_no_bodies", "holds no bodies");
    refused(plain.get_check("g_count", nullptr, 3, out), "g_count", "holds 8 bodies");
    refused(plain.get_check("g_range", outside, 2, out), "g_range", "indices[1] = 8");

    // ---- the row rules the kernel shares ----
    {
        double o[13];
        std::vector<double> r = rows_of(1);
        r[0] = 4.0, r[1] = 2.0, r[5] = 4.0, r[9] = 8.0;
        if (resolve_mass_row(r.data(), XPBD_MASS_DIRECT, o) != kMassRowOk || o[0] != 0.25 || o[1] != 0.5 || o[5] != 0.25 || o[9] != 0.125 || o[2] != 0.0 ||
            o[10] != 0.1 || o[12] != 0.3 || mass_row_fixed(o))
            ++failures;
        if (resolve_mass_row(r.data(), XPBD_MASS_INVERSE, o) != kMassRowOk || std::memcmp(o, r.data(), sizeof o) != 0)
            ++failures;
        const double zeros[13] = {0.0, -0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 2.0, 3.0};
        if (resolve_mass_row(zeros, XPBD_MASS_INVERSE, o) != kMassRowOk || !mass_row_fixed(o))
            ++failures;
    }

    if (failures)
        return 1;
    std::printf("%d checks ok\n", calls);
    return 0;
}
