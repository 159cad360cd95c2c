// CPU mirror of the speed buckets of the flat list's y-moving plane runs (tests/test_speed_buckets.py): their layout, through the
// library's own rayz_amd/csrc/plane_runs.hpp, and the bucket form of the f32 reject test as the device runs it.
// Built by the test with g++ -ffp-contract=off: every fm() below is one std::fma, as on the GPU.
//   layout <spheres>                     -> the mov-Y class's runs (rayz_plane::plan_runs) and, per run, its slot order, buckets
//                                           and remainder (rayz_plane::plan_buckets)
//   audit <spheres> <rays> <S> <f64>     -> every ray against every sphere of a bucket: the bucket form and the parent's
//                                           4-field plane form against the f64 discriminant
//   pairs <spheres> <rays> <S> <f64>     -> ray i against sphere i alone, as a member of a bucket whose speed lies the whole
//                                           allowed r / 16 off the sphere's (above it for even i, below for odd)
//   discs <records> <f64>                -> per RAYZ_KAT_BUCKET_DISCS record (its padded r2b at [28..31]) the bucket form of its
//                                           four spheres, a pad slot's value at their place, K2: 9 raw f32 on stdout
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

struct Basis { float e1x, e1z, e2x, e2y, e2z, k1, k2; };
static Basis make_basis(const float* ud, const float* o) { // flat_scan.hpp: make_basis<float>
    Basis b;
    const float h2 = fm(ud[2], ud[2], ud[0] * ud[0]);
    b.e1x = 1.0f, b.e1z = 0.0f;
    if (h2 > 1e-30f) {
        const float ih = 1.0f / std::sqrt(h2);
        b.e1x = ud[2] * ih;
        b.e1z = -(ud[0] * ih);
    }
    b.e2x = ud[1] * b.e1z;
    b.e2y = fm(ud[2], b.e1x, -(ud[0] * b.e1z));
    b.e2z = -(ud[1] * b.e1x);
    b.k1 = -fm(o[2], b.e1z, o[0] * b.e1x);
    b.k2 = -fm(o[2], b.e2z, fm(o[1], b.e2y, o[0] * b.e2x));
    return b;
}
static Basis ray_basis(const double* o3, const double* d3, bool f64_rays) { // the ray as the f32 / f64 kernel hands it to the filter
    float ud[3];
    if (f64_rays) {
        double u64[3];
        unit<double>(d3, u64);
        for (int j = 0; j < 3; ++j) ud[j] = (float)u64[j];
    } else {
        unit<float>(d3, ud);
    }
    const float o[3] = {(float)o3[0], (float)o3[1], (float)o3[2]};
    return make_basis(ud, o);
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

// flat_scan.hpp: bucket_k2, then ScanGroup<float, 3>::discs
static float bucket_k2(float v0, float cy, float ft, const Basis& b) { return fm(v0, ft * b.e2y, fm(cy, b.e2y, b.k2)); }
static float bucket_disc(const Basis& b, float K2, float cx, float cz, float r2b) {
    float p1 = fm(cx, b.e1x, b.k1), p2 = fm(cx, b.e2x, K2);
    p1 = fm(cz, b.e1z, p1);
    p2 = fm(cz, b.e2z, p2);
    return fm(-p1, p1, fm(-p2, p2, r2b));
}
// the parent's form of the same sphere: ScanGroup<float, 4>::discs
static float run_disc(const Basis& b, float cy, float ft, float cx, float cz, float vy, float r2) {
    const float K2 = fm(cy, b.e2y, b.k2);
    float p1 = fm(cx, b.e1x, b.k1), p2 = fm(cx, b.e2x, K2);
    p1 = fm(cz, b.e1z, p1);
    p2 = fm(cz, b.e2z, p2);
    p2 = fm(vy, ft * b.e2y, p2);
    return fm(-p1, p1, fm(-p2, p2, r2));
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

static int discs(const char* path, bool f64_rays) {
    const std::vector<double> rec = read_rows(path);
    for (size_t i = 0; i + 48 <= rec.size(); i += 48) {
        const double* a = &rec[i];
        const Basis b = ray_basis(a + 20, a + 23, f64_rays);
        const float K2 = bucket_k2((float)a[27], (float)a[4], (float)a[26], b);
        float out[9];
        for (int k = 0; k < 4; ++k) {
            out[k] = bucket_disc(b, K2, (float)a[k], (float)a[8 + k], (float)a[28 + k]);
            out[4 + k] = bucket_disc(b, K2, (float)a[k], (float)a[8 + k], -INFINITY);
        }
        out[8] = K2;
        std::fwrite(out, sizeof(float), 9, stdout);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string cmd = argv[1];
    if (cmd == "discs") return argc < 4 ? 2 : discs(argv[2], std::atoi(argv[3]) != 0);
    const std::vector<double> sph = read_rows(argv[2]);
    const size_t ns = sph.size() / 7;
    std::vector<uint32_t> movy;
    for (uint32_t i = 0; i < ns; ++i) {
        const double* s = &sph[7 * i];
        if (s[3] == 0 && s[5] == 0 && s[4] != 0) movy.push_back(i); // rayz_hip.hip: velocity_class
    }
    auto cy_of = [&](uint32_t pool) { return (float)sph[7 * pool + 1]; };
    auto vy_of = [&](uint32_t pool) { return (float)sph[7 * pool + 4]; };
    auto r_of = [&](uint32_t pool) { return std::fabs(sph[7 * pool + 6]); };
    std::vector<rayz_plane::PlaneRun> runs;
    std::vector<std::vector<uint32_t>> members;
    std::vector<uint32_t> loose;
    const uint32_t slots = rayz_plane::plan_runs(movy, cy_of, 4, runs, members, loose);
    std::vector<rayz_plane::RunBuckets> rb;
    for (const auto& m : members) rb.push_back(rayz_plane::plan_buckets(m, vy_of, r_of, 4));
    if (cmd == "layout") {
        std::printf("{\"plane_slots\": %u, \"runs\": [", slots);
        for (size_t j = 0; j < runs.size(); ++j) {
            std::printf("%s{\"cy_bits\": %u, \"first\": %u, \"end\": %u, \"members\": [", j ? ", " : "", rayz_plane::bits32(runs[j].cy),
                        runs[j].first, runs[j].end);
            for (size_t k = 0; k < members[j].size(); ++k) std::printf("%s%u", k ? ", " : "", members[j][k]);
            std::printf("], \"order\": [");
            for (size_t k = 0; k < rb[j].order.size(); ++k) std::printf("%s%u", k ? ", " : "", rb[j].order[k]);
            std::printf("], \"bucketed\": %u, \"buckets\": [", rb[j].bucketed);
            uint32_t at = 0;
            for (size_t q = 0; q < rb[j].count.size(); ++q) {
                std::printf("%s{\"v0_bits\": %u, \"first\": %u, \"end\": %u}", q ? ", " : "", rayz_plane::bits32(rb[j].v0[q]),
                            runs[j].first + at, runs[j].first + at + rb[j].count[q]);
                at += rb[j].count[q];
            }
            std::printf("]}");
        }
        std::printf("]}\n");
        return 0;
    }
    if (argc < 6) return 2;
    const std::vector<double> rays = read_rows(argv[3]);
    const double S = std::atof(argv[4]);
    const bool f64_rays = std::atoi(argv[5]) != 0;
    unsigned long long pairs = 0, hits = 0, cands = 0, parent = 0, fneg = 0, pad_pass = 0;
    if (cmd == "pairs") {
        for (size_t i = 0; i < ns && 7 * i + 7 <= rays.size(); ++i) {
            const double *s = &sph[7 * i], *ry = &rays[7 * i];
            const float vy = (float)s[4], v0 = (float)(s[4] + (i % 2 ? -1.0 : 1.0) * std::fabs(s[6]) / rayz_plane::kBucketCap);
            const Basis b = ray_basis(ry, ry + 3, f64_rays);
            const float ft = (float)ry[6], K2 = bucket_k2(v0, (float)s[1], ft, b);
            const bool cand = bucket_disc(b, K2, (float)s[0], (float)s[2], pad_r2b(s, S, f64_rays, v0)) >= 0.0f;
            const bool hit = f64_hit(s, ry, f64_rays);
            pad_pass += bucket_disc(b, K2, (float)s[0], (float)s[2], -INFINITY) >= 0.0f;
            parent += run_disc(b, (float)s[1], ft, (float)s[0], (float)s[2], vy, pad_r2(s, S, f64_rays)) >= 0.0f;
            ++pairs, hits += hit, cands += cand, fneg += hit && !cand;
        }
    } else {
        struct Member { uint32_t pool; float v0, cy, r2b, r2; };
        std::vector<Member> mem;
        for (size_t j = 0; j < runs.size(); ++j) {
            size_t at = 0;
            for (size_t q = 0; q < rb[j].count.size(); ++q)
                for (uint32_t k = 0; k < rb[j].count[q]; ++k, ++at) {
                    const uint32_t pool = rb[j].order[at];
                    mem.push_back({pool, rb[j].v0[q], runs[j].cy, pad_r2b(&sph[7 * pool], S, f64_rays, rb[j].v0[q]), pad_r2(&sph[7 * pool], S, f64_rays)});
                }
        }
        for (size_t k = 0; k + 7 <= rays.size(); k += 7) {
            const double* ry = &rays[k];
            const Basis b = ray_basis(ry, ry + 3, f64_rays);
            const float ft = (float)ry[6];
            float v0 = NAN, cy = NAN, K2 = 0;
            for (const Member& m : mem) {
                const double* s = &sph[7 * m.pool];
                if (!(m.v0 == v0 && m.cy == cy)) v0 = m.v0, cy = m.cy, K2 = bucket_k2(v0, cy, ft, b); // once per ray and bucket
                const bool cand = bucket_disc(b, K2, (float)s[0], (float)s[2], m.r2b) >= 0.0f;
                const bool hit = f64_hit(s, ry, f64_rays);
                pad_pass += bucket_disc(b, K2, (float)s[0], (float)s[2], -INFINITY) >= 0.0f;
                parent += run_disc(b, cy, ft, (float)s[0], (float)s[2], (float)s[4], m.r2) >= 0.0f;
                ++pairs, hits += hit, cands += cand, fneg += hit && !cand;
            }
        }
    }
    std::printf("{\"pairs\": %llu, \"f64_hits\": %llu, \"candidates\": %llu, \"parent_candidates\": %llu, \"false_negatives\": %llu, "
                "\"pad_passes\": %llu}\n", pairs, hits, cands, parent, fneg, pad_pass);
    return 0;
}
