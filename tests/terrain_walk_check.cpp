// Stand-alone host program of tests/test_terrain_walk_host.py: the terrain walk of the scene queries (terrain_cast<false> in
// constraint_solver_amd/csrc/xpbd_terrain_query.hip, whose routines up to terrain_cast are host code too) against the brute-force
// minimum over all triangles (terrain_cast<true>), bit for bit in t and the triangle, for random and crafted rays on several
// fields.  It is the place where a walk that does not end shows without a GPU: the test runs it under a time limit.  Built with
// the host side of hipcc only, under AddressSanitizer and UBSan; prints one line and returns 0 iff nothing differs.
#include "xpbd_terrain_query.hip"

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

using namespace xpbd;

// k_terrain_planes on the host: the header's formulas, operation by operation.
static std::vector<double> planes_of(const Terrain &t, const std::vector<double> &H)
{
    std::vector<double> out((size_t)(t.nx - 1) * (t.ny - 1) * 8);
    for (uint32_t j = 0; j + 1 < t.ny; ++j)
        for (uint32_t i = 0; i + 1 < t.nx; ++i) {
            const double *row = H.data() + (size_t)j * t.nx + i;
            const double h00 = row[0], h10 = row[1], h01 = row[t.nx], h11 = row[t.nx + 1];
            const Vec3 corner{t.x0 + (double)i * t.dx, t.y0 + (double)j * t.dy, h00};
            double *o = out.data() + ((size_t)j * (t.nx - 1) + i) * 8;
            for (uint32_t upper = 0; upper < 2; ++upper) {
                const double sx = upper ? (h11 - h01) / t.dx : (h10 - h00) / t.dx;
                const double sy = upper ? (h01 - h00) / t.dy : (h11 - h10) / t.dy;
                const Vec3 raw{-sx, -sy, 1.0};
                const Vec3 n = raw * (1.0 / length(raw));
                o[4 * upper] = n.x, o[4 * upper + 1] = n.y, o[4 * upper + 2] = n.z, o[4 * upper + 3] = dot(n, corner);
            }
        }
    return out;
}

int main()
{
    struct Field {
        uint32_t nx, ny;
        double x0, y0, dx, dy;
    } fields[] = {{2, 2, -1.0, 2.0, 0.5, 0.25}, {5, 4, -1.0, 2.0, 0.5, 0.25}, {9, 7, -3.1, -2.3, 0.7, 0.9}, {65, 65, -8.0, -8.0, 0.25, 0.25},
                  {33, 17, 1e6, -1e6, 0.1, 0.3}};
    std::mt19937_64 rng(7);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    long total = 0, bad = 0, hits = 0, at_infinity = 0, tiny = 0;
    for (const Field &f : fields) {
        Terrain t{nullptr, f.x0, f.y0, f.dx, f.dy, f.nx, f.ny};
        std::vector<double> H((size_t)f.nx * f.ny);
        for (uint32_t j = 0; j < f.ny; ++j)
            for (uint32_t i = 0; i < f.nx; ++i)
                H[(size_t)j * f.nx + i] = 0.6 * std::sin(0.9 * i + 0.3) * std::cos(0.7 * j);
        const std::vector<double> planes = planes_of(t, H);
        t.planes = planes.data();
        const double w = (f.nx - 1) * f.dx, h = (f.ny - 1) * f.dy;
        const bool big = f.nx * f.ny > 1000;
        std::vector<Line> rays;
        auto add = [&](Vec3 o, Vec3 d, double tmax = INFINITY) { rays.push_back(Line{o, d, tmax}); };
        for (int k = 0; k < (big ? 600 : 2000); ++k) { // random, every fourth one grazing as well
            const Vec3 o{f.x0 - 0.3 * w + 1.6 * w * U(rng), f.y0 - 0.3 * h + 1.6 * h * U(rng), -1.0 + 5.0 * U(rng)};
            const Vec3 d{N(rng), N(rng), N(rng) - 0.5};
            const double m[3] = {INFINITY, 3.0, 10.0};
            add(o, d, m[k % 3]);
            if (k % 4 == 0)
                add(o, Vec3{d.x, d.y, 0.02 * d.z});
        }
        const uint32_t stride = big ? 7 : 1; // corners, grid lines, diagonals, verticals
        for (uint32_t j = 0; j < f.ny; j += stride)
            for (uint32_t i = 0; i < f.nx; i += stride) {
                const double x = f.x0 + i * f.dx, y = f.y0 + j * f.dy;
                add(Vec3{x, y, 3.0}, Vec3{0, 0, -1});
                add(Vec3{x, y, -3.0}, Vec3{0, 0, 1});
                add(Vec3{x - f.dx, y - f.dy, 2.0}, Vec3{f.dx, f.dy, -0.7});
                add(Vec3{x + f.dx, y - f.dy, 2.0}, Vec3{-f.dx, f.dy, -0.7});
                add(Vec3{x - 3 * f.dx, y, 1.0}, Vec3{1, 0, -0.05});
                add(Vec3{x, y + 3 * f.dy, 1.0}, Vec3{0, -1, -0.05});
                add(Vec3{x - 3 * f.dx, y, -0.2}, Vec3{1, 0, 0});
                add(Vec3{x + 0.5 * f.dx, y, 3.0}, Vec3{0, 0, -1});
                add(Vec3{x, y + 0.5 * f.dy, 3.0}, Vec3{0, 0, -1});
                add(Vec3{x, y, 1.0}, Vec3{1, 1, -0.3});
                add(Vec3{x, y, 1.0}, Vec3{-1, -0.5, -0.3});
            }
        const double far = std::ldexp(1.0, 60); // origins so far away that successive borders get the same t
        add(Vec3{-far, f.y0 + 0.4 * h, 1.0}, Vec3{1, 0, 0});
        add(Vec3{-far, -far, 0.1}, Vec3{1, 1, 0});
        add(Vec3{f.x0 + 0.3 * w, far, far}, Vec3{0, -1, -1});
        add(Vec3{far, f.y0 + 0.4 * h, -0.5}, Vec3{-1, 0, 0});
        add(Vec3{f.x0 + 0.3 * w, f.y0 + 0.3 * h, far}, Vec3{0, 0, -1});
        add(Vec3{f.x0 - 1.0, f.y0 + 0.3 * h, -0.4}, Vec3{1, 0, 0}); // the outer wall below the surface
        add(Vec3{f.x0 - 1.0, f.y0 + 0.3 * h, -0.4}, Vec3{1, 0, 0}, 0.5);
        add(Vec3{f.x0 - 1.0, f.y0 - 1.0, 0.0}, Vec3{0, 0, -1});
        // direction components so small that a border's t overflows to +inf: in x, in y, in both, either sign; from over the
        // field (hitting: down, and missing: up), from under ground, from beside the field (every cell then begins at t = +inf)
        const size_t first_tiny = rays.size();
        const double small[3] = {5e-324, 1e-320, 1e-306};
        const Vec3 from[5] = {Vec3{f.x0 + 0.3 * w, f.y0 + 0.3 * h, 2.0}, Vec3{f.x0 + 0.125 * f.dx, f.y0 + 0.7 * f.dy, 2.0},
                              Vec3{f.x0 + 0.3 * w, f.y0 + 0.3 * h, -2.0}, Vec3{f.x0 - 1.0, f.y0 + 0.3 * h, 2.0}, Vec3{f.x0 + w, f.y0, 2.0}};
        for (const Vec3 &o : from)
            for (double e : small)
                for (double sign : {1.0, -1.0})
                    for (double dz : {-1.0, 1.0, 0.0}) {
                        add(o, Vec3{sign * e, 0.0, dz});
                        add(o, Vec3{0.0, sign * e, dz});
                        add(o, Vec3{sign * e, -sign * e, dz});
                        add(o, Vec3{sign * e, 0.25, dz});
                        add(o, Vec3{sign * e, sign * e, dz}, 10.0);
                    }
        for (size_t k = 0; k < rays.size(); ++k) {
            const Line &r = rays[k];
            if (r.d.x == 0.0 && r.d.y == 0.0 && r.d.z == 0.0)
                continue; // (not a ray: the kernels never cast it)
            const TerrainBest a = terrain_cast<false>(t, r, INFINITY), b = terrain_cast<true>(t, r, INFINITY);
            ++total;
            tiny += k >= first_tiny;
            hits += b.tri != kNoTriangle;
            at_infinity += b.tri != kNoTriangle && !(b.t < INFINITY);
            bool differs = a.tri != b.tri || std::memcmp(&a.t, &b.t, 8) != 0;
            if (!differs && b.tri != kNoTriangle && b.t > 0.0) { // a walk bounded by the hit's own distance still finds it
                const TerrainBest c = terrain_cast<false>(t, r, b.t);
                differs = c.tri != b.tri || c.t != b.t;
            }
            if (differs && ++bad < 10)
                std::printf("field %ux%u ray o=(%.17g %.17g %.17g) d=(%.17g %.17g %.17g) tmax %g: walk (%.17g, %u) brute (%.17g, %u)\n", f.nx, f.ny,
                            r.o.x, r.o.y, r.o.z, r.d.x, r.d.y, r.d.z, r.tmax, a.t, a.tri, b.t, b.tri);
        }
    }
    std::printf("%ld rays (%ld with a tiny direction component), %ld hits (%ld at t = +inf), %ld mismatches\n", total, tiny, hits, at_infinity, bad);
    return bad != 0;
}
