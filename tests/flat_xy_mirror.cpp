// CPU mirror of the flat list's reject test in its XY basis (flat_scan.hpp: kBasisXY; trace_kernels_flat.hpp: flat_xy_kernel) and of the
// host's choice between the two bases (rayz_amd/csrc/plane_runs.hpp: scan_price), for tests/test_flat_xy.py and
// tests/test_flat_xy_gpu.py.  Built by the tests with g++ -ffp-contract=off: every fm() below is one std::fma, as on the GPU.
//   price <plane_static> <bucket> <plane_movy> <loose_static> <loose_movy> <movg>   -> both prices and the form chosen
//   form <spheres>                       -> the pool's layout (plan_runs, plan_buckets), its slots by form, prices, the form chosen
//   audit <spheres> <rays> <S> <f64>     -> every ray against every sphere, each sphere in the form its place in the layout gives it
//                                           (run: 5 FMAs, bucket: 5, mov-Y remainder: 7, loose: 7 / 9, general velocity: 12), XY and
//                                           XZ basis, against the f64 discriminant
//   pairs <spheres> <rays> <S> <f64>     -> ray i against sphere i alone, in EVERY form its velocity class can take (its own height
//                                           as the run's; a bucket whose speed lies the whole r / 16 off its own)
//   discs <records> <f64> <op>           -> per RAYZ_KAT_SCAN_DISCS_XY (11) / RAYZ_KAT_BUCKET_DISCS_XY (12) record (padded r2 at
//                                           [28..31]): disc[4] k1 k2 e1x e1y, 8 raw f32 on stdout
// spheres: rows of 7 doubles (cx cy cz vx vy vz r); rays: rows of 7 doubles (ox oy oz dx dy dz time).
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../rayz_amd/csrc/plane_runs.hpp"

static std::vector<double> read_rows(const char* path) {
    std::vector<double> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) std::exit(2);
    double x;
    while (std::fread(&x, sizeof x, 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}

template <class R> static R fm(R a, R b, R c) { return std::fma(a, b, c); }

template <class R> static void unit(const double* d, R* u) { // device_math.hpp: unit(d) in R
    const R x = (R)d[0], y = (R)d[1], z = (R)d[2];
    const R m = std::sqrt(fm(z, z, fm(y, y, x * x)));
    const R inv = R(1) / m;
    u[0] = x * inv, u[1] = y * inv, u[2] = z * inv;
}

// e1 = (e1x, e1w, 0) in the XY basis (e1w = e1y), (e1x, 0, e1w) in the XZ basis (e1w = e1z)
struct Basis { float e1x, e1w, e2x, e2y, e2z, k1, k2; };
static Basis make_basis_xy(const float* ud, const float* o) { // flat_scan.hpp: make_basis<float, kBasisXY>
    Basis b;
    const float h2 = fm(ud[1], ud[1], ud[0] * ud[0]);
    b.e1x = 1.0f, b.e1w = 0.0f;
    if (h2 > 1e-30f) {
        const float ih = 1.0f / std::sqrt(h2);
        b.e1x = ud[1] * ih;
        b.e1w = -(ud[0] * ih);
    }
    b.e2x = -(ud[2] * b.e1w);
    b.e2y = ud[2] * b.e1x;
    b.e2z = fm(ud[0], b.e1w, -(ud[1] * b.e1x));
    b.k1 = -fm(o[1], b.e1w, o[0] * b.e1x);
    b.k2 = -fm(o[2], b.e2z, fm(o[1], b.e2y, o[0] * b.e2x));
    return b;
}
static Basis make_basis_xz(const float* ud, const float* o) { // flat_scan.hpp: make_basis<float, kBasisXZ>
    Basis b;
    const float h2 = fm(ud[2], ud[2], ud[0] * ud[0]);
    b.e1x = 1.0f, b.e1w = 0.0f;
    if (h2 > 1e-30f) {
        const float ih = 1.0f / std::sqrt(h2);
        b.e1x = ud[2] * ih;
        b.e1w = -(ud[0] * ih);
    }
    b.e2x = ud[1] * b.e1w;
    b.e2y = fm(ud[2], b.e1x, -(ud[0] * b.e1w));
    b.e2z = -(ud[1] * b.e1x);
    b.k1 = -fm(o[2], b.e1w, o[0] * b.e1x);
    b.k2 = -fm(o[2], b.e2z, fm(o[1], b.e2y, o[0] * b.e2x));
    return b;
}
static void narrowed_ray(const double* o3, const double* d3, bool f64_rays, float* ud, float* o) { // the ray as the filter gets it
    if (f64_rays) {
        double u64[3];
        unit<double>(d3, u64);
        for (int j = 0; j < 3; ++j) ud[j] = (float)u64[j];
    } else {
        unit<float>(d3, ud);
    }
    for (int j = 0; j < 3; ++j) o[j] = (float)o3[j];
}

static float round_up32(double v) {
    float f = (float)v;
    if ((double)f < v) f = std::nextafter(f, INFINITY);
    return f;
}
static double norm3(const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
// rayz_hip.hip: pad_radius2_scan and pad_radius2_bucket
static float pad_r2(const double* s, double S, bool f64_rays) {
    const double E = (f64_rays ? 40.0 : 32.0) * 5.9604644775390625e-08 * (norm3(s) + norm3(s + 3) + std::fabs(s[6]) + S);
    const double rp = std::fabs(s[6]) + E;
    return round_up32(rp * rp);
}
static float pad_r2b(const double* s, double S, bool f64_rays, float v0) {
    const double vy = s[4], h0 = std::max(std::fabs(vy - (double)v0), std::fabs((double)(float)vy - (double)v0));
    const double h = h0 * (1.0 + 0x1p-50) + 1e-300;
    const double E = (f64_rays ? 40.0 : 32.0) * 5.9604644775390625e-08 * (norm3(s) + norm3(s + 3) + h + std::fabs(s[6]) + h + S);
    const double rp = std::fabs(s[6]) + h + E;
    return round_up32(rp * rp);
}

static float disc_of(float p1, float p2, float r2) { return fm(-p1, p1, fm(-p2, p2, r2)); }
// ---- the XY forms (flat_scan.hpp: plane_run_k1 / _k2, bucket_k1 / _k2, PackedGroup::discs(RayBasis<R, kBasisXY>), the
// general-velocity ScanGroup<R, 2>::disc), in the device's order of stages ----
static float run_k(float cy, float ey, float k) { return fm(cy, ey, k); }
static float bucket_k(float v0, float cy, float ft, float ey, float k) { return fm(v0, ft * ey, fm(cy, ey, k)); }
static float xy_plane(const Basis& b, float K1, float K2, float cx, float cz, float r2) { // run and bucket: 5 FMAs
    const float p1 = fm(cx, b.e1x, K1);
    const float p2 = fm(cz, b.e2z, fm(cx, b.e2x, K2));
    return disc_of(p1, p2, r2);
}
static float xy_plane_movy(const Basis& b, float K1, float K2, float ft, float cx, float cz, float vy, float r2) { // 7
    const float p1 = fm(vy, ft * b.e1w, fm(cx, b.e1x, K1));
    const float p2 = fm(vy, ft * b.e2y, fm(cz, b.e2z, fm(cx, b.e2x, K2)));
    return disc_of(p1, p2, r2);
}
static float xy_loose(const Basis& b, float cx, float cy, float cz, float r2) { // 7
    const float p1 = fm(cy, b.e1w, fm(cx, b.e1x, b.k1));
    const float p2 = fm(cz, b.e2z, fm(cy, b.e2y, fm(cx, b.e2x, b.k2)));
    return disc_of(p1, p2, r2);
}
static float xy_loose_movy(const Basis& b, float ft, float cx, float cy, float cz, float vy, float r2) { // 9
    const float p1 = fm(vy, ft * b.e1w, fm(cy, b.e1w, fm(cx, b.e1x, b.k1)));
    const float p2 = fm(vy, ft * b.e2y, fm(cz, b.e2z, fm(cy, b.e2y, fm(cx, b.e2x, b.k2))));
    return disc_of(p1, p2, r2);
}
static float xy_movg(const Basis& b, float ft, const float* c, const float* v, float r2) { // 12
    const float p1 = fm(v[1], ft * b.e1w, fm(v[0], ft * b.e1x, fm(c[1], b.e1w, fm(c[0], b.e1x, b.k1))));
    const float p2 = fm(v[2], ft * b.e2z, fm(v[1], ft * b.e2y, fm(v[0], ft * b.e2x, fm(c[2], b.e2z, fm(c[1], b.e2y, fm(c[0], b.e2x, b.k2))))));
    return disc_of(p1, p2, r2);
}
// ---- the XZ forms of the same places (tests/plane_filter_mirror.cpp, tests/bucket_mirror.cpp), for the candidate counts ----
static float xz_plane(const Basis& b, float K2, float cx, float cz, float r2) {
    float p1 = fm(cx, b.e1x, b.k1), p2 = fm(cx, b.e2x, K2);
    p1 = fm(cz, b.e1w, p1);
    p2 = fm(cz, b.e2z, p2);
    return disc_of(p1, p2, r2);
}
static float xz_plane_movy(const Basis& b, float K2, float ft, float cx, float cz, float vy, float r2) {
    float p1 = fm(cx, b.e1x, b.k1), p2 = fm(cx, b.e2x, K2);
    p1 = fm(cz, b.e1w, p1);
    p2 = fm(cz, b.e2z, p2);
    p2 = fm(vy, ft * b.e2y, p2);
    return disc_of(p1, p2, r2);
}
static float xz_loose(const Basis& b, float ft, float cx, float cy, float cz, float vy, bool movy, float r2) {
    float p1 = fm(cx, b.e1x, b.k1), p2 = fm(cx, b.e2x, b.k2);
    p1 = fm(cz, b.e1w, p1);
    p2 = fm(cy, b.e2y, p2);
    p2 = fm(cz, b.e2z, p2);
    if (movy) p2 = fm(vy, ft * b.e2y, p2);
    return disc_of(p1, p2, r2);
}
static float xz_movg(const Basis& b, float ft, const float* c, const float* v, float r2) {
    const float p1 = fm(v[2], ft * b.e1w, fm(v[0], ft * b.e1x, fm(c[2], b.e1w, fm(c[0], b.e1x, b.k1))));
    const float p2 = fm(v[2], ft * b.e2z, fm(v[1], ft * b.e2y, fm(v[0], ft * b.e2x, fm(c[2], b.e2z, fm(c[1], b.e2y, fm(c[0], b.e2x, b.k2))))));
    return disc_of(p1, p2, r2);
}

// flat_scan.hpp: narrow_eval's f64 discriminant on the pool's f64 sphere
static bool f64_hit(const double* s, const double* ry, bool f64_rays) {
    const float ft = (float)ry[6];
    double o[3], d[3];
    for (int j = 0; j < 3; ++j) o[j] = f64_rays ? ry[j] : (double)(float)ry[j], d[j] = f64_rays ? ry[3 + j] : (double)(float)ry[3 + j];
    const double tt = f64_rays ? ry[6] : (double)ft;
    const double a = fm(d[2], d[2], fm(d[1], d[1], d[0] * d[0]));
    const double qx = fm(s[3], tt, s[0] - o[0]), qy = fm(s[4], tt, s[1] - o[1]), qz = fm(s[5], tt, s[2] - o[2]);
    const double hb = fm(d[2], qz, fm(d[1], qy, d[0] * qx));
    const double cc = fm(qz, qz, fm(qy, qy, fm(qx, qx, -(s[6] * s[6]))));
    return fm(-a, cc, hb * hb) >= 0.0;
}

static int discs(const char* path, bool f64_rays, int op) {
    const std::vector<double> rec = read_rows(path);
    for (size_t i = 0; i + 48 <= rec.size(); i += 48) {
        const double* a = &rec[i];
        float ud[3], o[3];
        narrowed_ray(a + 20, a + 23, f64_rays, ud, o);
        Basis b = make_basis_xy(ud, o);
        const float ft = (float)a[26], cy = (float)a[4];
        float out[8];
        if (op == 12) {
            const float v0 = (float)a[27];
            b.k1 = bucket_k(v0, cy, ft, b.e1w, b.k1), b.k2 = bucket_k(v0, cy, ft, b.e2y, b.k2);
            for (int k = 0; k < 4; ++k) out[k] = xy_plane(b, b.k1, b.k2, (float)a[k], (float)a[8 + k], (float)a[28 + k]);
        } else {
            const int cls = (int)a[27];
            if (cls >= 2) b.k1 = run_k(cy, b.e1w, b.k1), b.k2 = run_k(cy, b.e2y, b.k2);
            for (int k = 0; k < 4; ++k) {
                const float cx = (float)a[k], cyk = (float)a[4 + k], cz = (float)a[8 + k], vy = (float)a[16 + k], r2 = (float)a[28 + k];
                out[k] = cls == 0 ? xy_loose(b, cx, cyk, cz, r2) : cls == 1 ? xy_loose_movy(b, ft, cx, cyk, cz, vy, r2)
                         : cls == 2 ? xy_plane(b, b.k1, b.k2, cx, cz, r2) : xy_plane_movy(b, b.k1, b.k2, ft, cx, cz, vy, r2);
            }
        }
        out[4] = b.k1, out[5] = b.k2, out[6] = b.e1x, out[7] = b.e1w;
        std::fwrite(out, sizeof(float), 8, stdout);
    }
    return 0;
}

static void print_price(const rayz_plane::ScanSlots& n) {
    std::printf("\"slots\": {\"plane_static\": %llu, \"bucket\": %llu, \"plane_movy\": %llu, \"loose_static\": %llu, \"loose_movy\": %llu, "
                "\"movg\": %llu}, \"price_xz\": %llu, \"price_xy\": %llu, \"form\": %u",
                (unsigned long long)n.plane_static, (unsigned long long)n.bucket, (unsigned long long)n.plane_movy,
                (unsigned long long)n.loose_static, (unsigned long long)n.loose_movy, (unsigned long long)n.movg,
                (unsigned long long)rayz_plane::scan_price(n, rayz_plane::kScanFormXZ),
                (unsigned long long)rayz_plane::scan_price(n, rayz_plane::kScanFormXY), rayz_plane::cheaper_scan_form(n));
}

enum Place { kRun, kBucket, kRemainder, kLoose, kLooseMovY, kMovG };
struct Member { uint32_t pool; Place place; float cy, v0, r2; };

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string cmd = argv[1];
    if (cmd == "price") {
        if (argc < 8) return 2;
        rayz_plane::ScanSlots n;
        n.plane_static = std::strtoull(argv[2], nullptr, 10), n.bucket = std::strtoull(argv[3], nullptr, 10);
        n.plane_movy = std::strtoull(argv[4], nullptr, 10), n.loose_static = std::strtoull(argv[5], nullptr, 10);
        n.loose_movy = std::strtoull(argv[6], nullptr, 10), n.movg = std::strtoull(argv[7], nullptr, 10);
        std::printf("{");
        print_price(n);
        std::printf("}\n");
        return 0;
    }
    if (cmd == "discs") return argc < 5 ? 2 : discs(argv[2], std::atoi(argv[3]) != 0, std::atoi(argv[4]));
    const std::vector<double> sph = read_rows(argv[2]);
    const size_t ns = sph.size() / 7;
    // the layout, as rayz_hip.hip: plan_slots makes it (groups of 4 in the packed classes, 2 in the general-velocity one)
    std::vector<uint32_t> cls[3];
    for (uint32_t i = 0; i < ns; ++i) {
        const double* s = &sph[7 * i];
        const bool x = s[3] != 0, y = s[4] != 0, z = s[5] != 0;
        cls[!x && !y && !z ? 0 : (!x && !z) ? 1 : 2].push_back(i);
    }
    auto cy_of = [&](uint32_t pool) { return (float)sph[7 * pool + 1]; };
    auto vy_of = [&](uint32_t pool) { return (float)sph[7 * pool + 4]; };
    auto r_of = [&](uint32_t pool) { return std::fabs(sph[7 * pool + 6]); };
    std::vector<rayz_plane::PlaneRun> runs[2];
    std::vector<std::vector<uint32_t>> members[2];
    std::vector<uint32_t> loose[2];
    uint32_t plane_slots[2], class_slots[2];
    for (int c = 0; c < 2; ++c) {
        plane_slots[c] = rayz_plane::plan_runs(cls[c], cy_of, 4, runs[c], members[c], loose[c]);
        class_slots[c] = plane_slots[c] + (uint32_t)(loose[c].size() + 7) / 8 * 8;
    }
    std::vector<rayz_plane::RunBuckets> rb;
    for (const auto& m : members[1]) rb.push_back(rayz_plane::plan_buckets(m, vy_of, r_of, 4));
    const rayz_plane::ScanSlots slots = rayz_plane::scan_slots(plane_slots, class_slots, rb, (uint32_t)(cls[2].size() + 3) / 4 * 4);
    if (cmd == "form") {
        std::printf("{\"runs\": [%zu, %zu], \"buckets\": %zu, ", runs[0].size(), runs[1].size(),
                    [&] { size_t n = 0; for (const auto& b : rb) n += b.count.size(); return n; }());
        print_price(slots);
        std::printf("}\n");
        return 0;
    }
    if (argc < 6) return 2;
    const std::vector<double> rays = read_rows(argv[3]);
    const double S = std::atof(argv[4]);
    const bool f64_rays = std::atoi(argv[5]) != 0;
    unsigned long long pairs = 0, hits = 0, cands = 0, parent = 0, fneg = 0, parent_fneg = 0, pad_pass = 0;
    const float ninf = -INFINITY;
    auto tally = [&](bool hit, float xy, float xz, float pad) {
        ++pairs, hits += hit, cands += xy >= 0.0f, parent += xz >= 0.0f, fneg += hit && !(xy >= 0.0f), parent_fneg += hit && !(xz >= 0.0f);
        pad_pass += pad >= 0.0f;
    };
    if (cmd == "pairs") {
        for (size_t i = 0; i < ns && 7 * i + 7 <= rays.size(); ++i) {
            const double *s = &sph[7 * i], *ry = &rays[7 * i];
            float ud[3], o[3];
            narrowed_ray(ry, ry + 3, f64_rays, ud, o);
            const Basis b = make_basis_xy(ud, o), z = make_basis_xz(ud, o);
            const float ft = (float)ry[6], c[3] = {(float)s[0], (float)s[1], (float)s[2]}, v[3] = {(float)s[3], (float)s[4], (float)s[5]};
            const float r2 = pad_r2(s, S, f64_rays);
            const bool hit = f64_hit(s, ry, f64_rays);
            const float K1 = run_k(c[1], b.e1w, b.k1), K2 = run_k(c[1], b.e2y, b.k2), Z2 = run_k(c[1], z.e2y, z.k2);
            const bool still = s[3] == 0 && s[4] == 0 && s[5] == 0, movy = s[3] == 0 && s[5] == 0 && !still;
            if (still) {
                tally(hit, xy_plane(b, K1, K2, c[0], c[2], r2), xz_plane(z, Z2, c[0], c[2], r2), xy_plane(b, K1, K2, c[0], c[2], ninf));
                tally(hit, xy_loose(b, c[0], c[1], c[2], r2), xz_loose(z, ft, c[0], c[1], c[2], 0.0f, false, r2), xy_loose(b, c[0], c[1], c[2], ninf));
            }
            if (movy) {
                const float v0 = (float)(s[4] + (i % 2 ? -1.0 : 1.0) * std::fabs(s[6]) / rayz_plane::kBucketCap), r2b = pad_r2b(s, S, f64_rays, v0);
                const float B1 = bucket_k(v0, c[1], ft, b.e1w, b.k1), B2 = bucket_k(v0, c[1], ft, b.e2y, b.k2), Zb = bucket_k(v0, c[1], ft, z.e2y, z.k2);
                tally(hit, xy_plane(b, B1, B2, c[0], c[2], r2b), xz_plane(z, Zb, c[0], c[2], r2b), xy_plane(b, B1, B2, c[0], c[2], ninf));
                tally(hit, xy_plane_movy(b, K1, K2, ft, c[0], c[2], v[1], r2), xz_plane_movy(z, Z2, ft, c[0], c[2], v[1], r2),
                      xy_plane_movy(b, K1, K2, ft, c[0], c[2], 0.0f, ninf));
                tally(hit, xy_loose_movy(b, ft, c[0], c[1], c[2], v[1], r2), xz_loose(z, ft, c[0], c[1], c[2], v[1], true, r2),
                      xy_loose_movy(b, ft, c[0], c[1], c[2], 0.0f, ninf));
            }
            tally(hit, xy_movg(b, ft, c, v, r2), xz_movg(z, ft, c, v, r2), xy_movg(b, ft, c, v, ninf)); // (any sphere fits the general form)
        }
    } else if (cmd == "audit") {
        std::vector<Member> mem;
        for (size_t j = 0; j < runs[0].size(); ++j)
            for (uint32_t pool : members[0][j]) mem.push_back({pool, kRun, runs[0][j].cy, 0.0f, pad_r2(&sph[7 * pool], S, f64_rays)});
        for (size_t j = 0; j < runs[1].size(); ++j) {
            size_t at = 0;
            for (size_t q = 0; q < rb[j].count.size(); ++q)
                for (uint32_t k = 0; k < rb[j].count[q]; ++k, ++at)
                    mem.push_back({rb[j].order[at], kBucket, runs[1][j].cy, rb[j].v0[q], pad_r2b(&sph[7 * rb[j].order[at]], S, f64_rays, rb[j].v0[q])});
            for (; at < rb[j].order.size(); ++at) mem.push_back({rb[j].order[at], kRemainder, runs[1][j].cy, 0.0f, pad_r2(&sph[7 * rb[j].order[at]], S, f64_rays)});
        }
        for (uint32_t pool : loose[0]) mem.push_back({pool, kLoose, 0.0f, 0.0f, pad_r2(&sph[7 * pool], S, f64_rays)});
        for (uint32_t pool : loose[1]) mem.push_back({pool, kLooseMovY, 0.0f, 0.0f, pad_r2(&sph[7 * pool], S, f64_rays)});
        for (uint32_t pool : cls[2]) mem.push_back({pool, kMovG, 0.0f, 0.0f, pad_r2(&sph[7 * pool], S, f64_rays)});
        for (size_t k = 0; k + 7 <= rays.size(); k += 7) {
            const double* ry = &rays[k];
            float ud[3], o[3];
            narrowed_ray(ry, ry + 3, f64_rays, ud, o);
            const Basis b = make_basis_xy(ud, o), z = make_basis_xz(ud, o);
            const float ft = (float)ry[6];
            for (const Member& m : mem) {
                const double* s = &sph[7 * m.pool];
                const float c[3] = {(float)s[0], (float)s[1], (float)s[2]}, v[3] = {(float)s[3], (float)s[4], (float)s[5]};
                const bool hit = f64_hit(s, ry, f64_rays);
                if (m.place == kRun || m.place == kRemainder) {
                    const float K1 = run_k(m.cy, b.e1w, b.k1), K2 = run_k(m.cy, b.e2y, b.k2), Z2 = run_k(m.cy, z.e2y, z.k2);
                    if (m.place == kRun) tally(hit, xy_plane(b, K1, K2, c[0], c[2], m.r2), xz_plane(z, Z2, c[0], c[2], m.r2), xy_plane(b, K1, K2, c[0], c[2], ninf));
                    else tally(hit, xy_plane_movy(b, K1, K2, ft, c[0], c[2], v[1], m.r2), xz_plane_movy(z, Z2, ft, c[0], c[2], v[1], m.r2),
                               xy_plane_movy(b, K1, K2, ft, c[0], c[2], 0.0f, ninf));
                } else if (m.place == kBucket) {
                    const float B1 = bucket_k(m.v0, m.cy, ft, b.e1w, b.k1), B2 = bucket_k(m.v0, m.cy, ft, b.e2y, b.k2), Zb = bucket_k(m.v0, m.cy, ft, z.e2y, z.k2);
                    tally(hit, xy_plane(b, B1, B2, c[0], c[2], m.r2), xz_plane(z, Zb, c[0], c[2], m.r2), xy_plane(b, B1, B2, c[0], c[2], ninf));
                } else if (m.place == kLoose) {
                    tally(hit, xy_loose(b, c[0], c[1], c[2], m.r2), xz_loose(z, ft, c[0], c[1], c[2], 0.0f, false, m.r2), xy_loose(b, c[0], c[1], c[2], ninf));
                } else if (m.place == kLooseMovY) {
                    tally(hit, xy_loose_movy(b, ft, c[0], c[1], c[2], v[1], m.r2), xz_loose(z, ft, c[0], c[1], c[2], v[1], true, m.r2),
                          xy_loose_movy(b, ft, c[0], c[1], c[2], 0.0f, ninf));
                } else {
                    tally(hit, xy_movg(b, ft, c, v, m.r2), xz_movg(z, ft, c, v, m.r2), xy_movg(b, ft, c, v, ninf));
                }
            }
        }
    } else {
        return 2;
    }
    std::printf("{\"pairs\": %llu, \"f64_hits\": %llu, \"candidates\": %llu, \"parent_candidates\": %llu, \"false_negatives\": %llu, "
                "\"parent_false_negatives\": %llu, \"pad_passes\": %llu}\n", pairs, hits, cands, parent, fneg, parent_fneg, pad_pass);
    return 0;
}
