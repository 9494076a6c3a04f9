// Stand-alone host program of tests/test_terrain_distance_walk_host.py: the ring walk of the terrain distance queries
// (terrain_distance_walk<false, 1> in constraint_solver_amd/csrc/xpbd_terrain_query.hip, whose routines up to the per-query walk and
// the record are host code too) against the brute-force minimum over every sample (terrain_distance_walk<true, 1>), in every byte of
// the 96-byte record, for points and unit cubes on five fields.  It is the place where a walk that does not end, or that stops a
// ring early, shows without a GPU: the test runs it under a time limit.  Built with the host side of hipcc only, under
// AddressSanitizer and UBSan; prints one line and returns 0 iff nothing differs.
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

// The shape table of one cube spanning [-h, h]^3: what the candidates read of PolytopeTables.
struct CubeTable {
    std::vector<double> verts, planes, centroids, radii;
    std::vector<uint32_t> face_start, face_verts, edges;
    ShapeDesc desc;
    PolytopeTables t;

    explicit CubeTable(double h)
    {
        for (int k = 0; k < 8; ++k) {
            const double v[3] = {(k == 1 || k == 2 || k == 5 || k == 6) ? h : -h, (k == 2 || k == 3 || k == 6 || k == 7) ? h : -h, k >= 4 ? h : -h};
            verts.insert(verts.end(), v, v + 3);
        }
        const uint32_t faces[6][4] = {{0, 3, 2, 1}, {4, 5, 6, 7}, {0, 1, 5, 4}, {2, 3, 7, 6}, {0, 4, 7, 3}, {1, 2, 6, 5}}; // -z +z -y +y -x +x
        const double normals[6][3] = {{0, 0, -1}, {0, 0, 1}, {0, -1, 0}, {0, 1, 0}, {-1, 0, 0}, {1, 0, 0}};
        for (int f = 0; f < 6; ++f) {
            face_start.push_back(4u * f);
            face_verts.insert(face_verts.end(), faces[f], faces[f] + 4);
            planes.insert(planes.end(), normals[f], normals[f] + 3);
            planes.push_back(h);
        }
        face_start.push_back(24u);
        const uint32_t e[12][2] = {{0, 1}, {0, 3}, {0, 4}, {1, 2}, {1, 5}, {2, 3}, {2, 6}, {3, 7}, {4, 5}, {4, 7}, {5, 6}, {6, 7}};
        for (auto &x : e)
            edges.insert(edges.end(), x, x + 2);
        centroids = {0.0, 0.0, 0.0};
        radii = {std::sqrt(3.0 * h * h)};
        desc = ShapeDesc{0, 8, 0, 6, 0, 12, 0, 0};
        t = PolytopeTables{};
        t.verts = verts.data(), t.planes = planes.data(), t.centroids = centroids.data(), t.desc = &desc;
        t.face_start = face_start.data(), t.face_verts = face_verts.data(), t.edges = edges.data(), t.radii = radii.data();
        t.n_shapes = 1, t.total_verts = 8, t.max_verts = 8, t.max_faces = 6, t.max_face_verts = 4;
    }
};

template <bool BRUTE>
static xpbd_distance_hit answer(const TerrainHeights &tf, const PolytopeTables &t, const xpbd_distance_query &q, uint32_t *looked_at = nullptr)
{
    const DistanceVolume vol = load_distance_volume(t, q);
    Vec3 aw[XPBD_MAX_SHAPE_VERTS];
    DistanceBest best{INFINITY, kNoCandidate};
    if (vol.valid) {
        for (uint32_t v = 0; v < vol.da.n_verts; ++v)
            aw[v] = volume_vertex(t, vol, v);
        best = terrain_distance_walk<BRUTE, 1>(tf, t, vol, aw, 0, looked_at);
    }
    return terrain_distance_record(tf, t, vol, aw, best);
}

int main()
{
    struct Field {
        uint32_t nx, ny;
        double x0, y0, dx, dy;
        bool binary;
    } fields[] = {{2, 2, -1.0, 2.0, 0.5, 0.25, true}, {4, 3, -1.0, 2.0, 0.5, 0.25, true}, {9, 7, -3.1, -2.3, 0.7, 0.9, false},
                  {65, 65, -8.0, -8.0, 0.25, 0.25, false}, {33, 17, 1e6, -1e6, 0.1, 0.3, false}};
    std::mt19937_64 rng(11);
    std::uniform_real_distribution<double> U(0.0, 1.0);
    std::normal_distribution<double> N(0.0, 1.0);
    const CubeTable cube(0.5);
    long total = 0, bad = 0, overlaps = 0, misses = 0, by_feature[3] = {0, 0, 0};
    unsigned long long looked = 0, walks = 0;
    for (const Field &f : fields) {
        Terrain t{nullptr, f.x0, f.y0, f.dx, f.dy, f.nx, f.ny};
        std::vector<double> H((size_t)f.nx * f.ny);
        for (uint32_t j = 0; j < f.ny; ++j)
            for (uint32_t i = 0; i < f.nx; ++i) {
                const double h = 0.6 * std::sin(0.9 * i + 0.3) * std::cos(0.7 * j);
                H[(size_t)j * f.nx + i] = f.binary ? std::floor(h * 8.0) / 8.0 : h; // multiples of 1/8 on the binary fields
            }
        const std::vector<double> planes = planes_of(t, H);
        t.planes = planes.data();
        const TerrainHeights tf{t, H.data()};
        const double w = (f.nx - 1) * f.dx, h = (f.ny - 1) * f.dy;
        const bool big = f.nx * f.ny > 1000;
        std::vector<xpbd_distance_query> qs;
        auto add = [&](Vec3 p, Quat r, uint32_t shape, double dmax) {
            xpbd_distance_query q{};
            q.position[0] = p.x, q.position[1] = p.y, q.position[2] = p.z;
            q.rotation[0] = r.s, q.rotation[1] = r.x, q.rotation[2] = r.y, q.rotation[3] = r.z;
            q.max_distance = dmax, q.shape = shape, q.ignore_body = XPBD_NO_HIT, q.mask = ~0u;
            qs.push_back(q);
        };
        const Quat ident{1.0, 0.0, 0.0, 0.0};
        const double reach[3] = {0.0, f.dx > f.dy ? f.dx : f.dy, INFINITY};
        for (int k = 0; k < (big ? 150 : 600); ++k) { // random places over, in, under and beside the field; points and turned cubes
            const Vec3 p{f.x0 - 0.4 * w - 1.0 + (1.8 * w + 2.0) * U(rng), f.y0 - 0.4 * h - 1.0 + (1.8 * h + 2.0) * U(rng), -1.2 + 3.5 * U(rng)};
            Quat r{N(rng), N(rng), N(rng), N(rng)};
            const double len = std::sqrt(r.s * r.s + r.x * r.x + r.y * r.y + r.z * r.z);
            r = Quat{r.s / len, r.x / len, r.y / len, r.z / len};
            add(p, r, k % 2 ? 0u : XPBD_DISTANCE_POINT, reach[k % 3]);
            if (k % 5 == 0)
                add(p, ident, 0u, reach[(k / 5) % 3]);
        }
        const uint32_t stride = big ? 16 : 1; // centres exactly on samples, grid lines and the diagonal, at three heights
        for (uint32_t j = 0; j < f.ny; j += stride)
            for (uint32_t i = 0; i < f.nx; i += stride) {
                const double x = f.x0 + i * f.dx, y = f.y0 + j * f.dy, z = H[(size_t)j * f.nx + i];
                for (double dmax : reach) {
                    add(Vec3{x, y, z + 0.75}, ident, XPBD_DISTANCE_POINT, dmax);
                    add(Vec3{x, y, z}, ident, XPBD_DISTANCE_POINT, dmax);
                    add(Vec3{x + 0.5 * f.dx, y, z + 0.3}, ident, XPBD_DISTANCE_POINT, dmax);
                    add(Vec3{x + 0.5 * f.dx, y + 0.5 * f.dy, z + 0.3}, ident, XPBD_DISTANCE_POINT, dmax);
                    add(Vec3{x, y, z + 1.25}, ident, 0u, dmax);
                    add(Vec3{x, y + 0.5 * f.dy, z + 0.5625}, ident, 0u, dmax);
                }
            }
        // far beside and far above the field, the field's corners, and records that find nothing
        for (double dmax : reach) {
            add(Vec3{f.x0 - 50.0 * w - 100.0, f.y0 + 0.3 * h, 0.5}, ident, XPBD_DISTANCE_POINT, dmax);
            add(Vec3{f.x0 + 0.3 * w, f.y0 + 60.0 * h + 100.0, 0.5}, ident, 0u, dmax);
            add(Vec3{f.x0 + 51.0 * w + 100.0, f.y0 - 50.0 * h - 100.0, -3.0}, ident, 0u, dmax);
            add(Vec3{f.x0 + 0.3 * w, f.y0 + 0.6 * h, 1.0e4}, ident, XPBD_DISTANCE_POINT, dmax);
            add(Vec3{f.x0 + 0.6 * w, f.y0 + 0.3 * h, 1.0e4}, ident, 0u, dmax);
            add(Vec3{f.x0, f.y0, 1.0}, ident, XPBD_DISTANCE_POINT, dmax);
            add(Vec3{f.x0 + w, f.y0 + h, 1.0}, ident, XPBD_DISTANCE_POINT, dmax);
            add(Vec3{f.x0 + w, f.y0, 1.5}, ident, 0u, dmax);
            add(Vec3{f.x0 - 0.5, f.y0 + h + 0.5, 0.0}, ident, 0u, dmax);
        }
        add(Vec3{f.x0, f.y0, 1.0}, ident, 7u, INFINITY);
        add(Vec3{f.x0, f.y0, 1.0}, ident, XPBD_DISTANCE_POINT, -1.0);
        add(Vec3{f.x0, f.y0, 1.0}, ident, XPBD_DISTANCE_POINT, NAN);
        add(Vec3{NAN, f.y0, 1.0}, ident, XPBD_DISTANCE_POINT, INFINITY);
        add(Vec3{f.x0, INFINITY, 1.0}, ident, 0u, INFINITY);
        add(Vec3{f.x0, f.y0, 1.0}, Quat{NAN, 0.0, 0.0, 0.0}, 0u, 1.0);
        for (const xpbd_distance_query &q : qs) {
            uint32_t seen = 0;
            const xpbd_distance_hit a = answer<false>(tf, cube.t, q, &seen), b = answer<true>(tf, cube.t, q);
            ++total;
            looked += seen, walks += 1;
            overlaps += b.body == XPBD_HIT_TERRAIN && b.feature == XPBD_DISTANCE_OVERLAP;
            misses += b.body == XPBD_NO_HIT;
            if (b.body == XPBD_HIT_TERRAIN && b.feature < 3u)
                ++by_feature[b.feature];
            if (std::memcmp(&a, &b, sizeof a) != 0 && ++bad < 10)
                std::printf("field %ux%u query p=(%.17g %.17g %.17g) q=(%.17g %.17g %.17g %.17g) shape %u dmax %g: walk (%u %u %u %u %.17g) brute (%u %u %u "
                            "%u %.17g)\n",
                            f.nx, f.ny, q.position[0], q.position[1], q.position[2], q.rotation[0], q.rotation[1], q.rotation[2], q.rotation[3],
                            q.shape, q.max_distance, a.body, a.feature, a.index_a, a.index_b, a.distance, b.body, b.feature, b.index_a, b.index_b,
                            b.distance);
        }
    }
    std::printf("%ld queries (FACE_A %ld, FACE_B %ld, EDGES %ld, overlaps %ld, misses %ld), %.1f samples per walk, %ld mismatches\n", total, by_feature[0],
                by_feature[1], by_feature[2], overlaps, misses, (double)looked / (double)walks, bad);
    return bad != 0;
}
