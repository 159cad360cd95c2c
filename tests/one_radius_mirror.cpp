// CPU mirror of the one-radius sets of the flat list's plane runs and speed buckets (tests/test_one_radius.py): their layout,
// through the library's own rayz_amd/csrc/plane_runs.hpp, and the set form of the f32 reject test (xy basis) as the device runs it.
// Built by the test with g++ -ffp-contract=off: every fm() below is one std::fma, as on the GPU.
//   layout <spheres>                 -> per class (static, mov-Y) its runs, their slot order, buckets and one-radius sets
//   audit <spheres> <rays> <S> <f64> -> every ray against every member of a set: the set form, the XY form the member had before
//                                       (its own padded r², or its bucket's r2b) and the f64 discriminant; and the set's R2 (the
//                                       library's class_set_r2) against each member's own padded square
//   discs <records> <f64>            -> per RAYZ_KAT_SET_DISCS record (its padded R2 at [36]) the set form of its eight spheres,
//                                       K1, K2: 10 raw f32 on stdout
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

struct Basis { float e1x, e1y, e2x, e2y, e2z, k1, k2; };
static Basis make_basis(const float* ud, const float* o) { // flat_scan.hpp: make_basis<float, kBasisXY>
    Basis b;
    const float h2 = fm(ud[1], ud[1], ud[0] * ud[0]);
    b.e1x = 1.0f, b.e1y = 0.0f;
    if (h2 > 1e-30f) {
        const float ih = 1.0f / std::sqrt(h2);
        b.e1x = ud[1] * ih;
        b.e1y = -(ud[0] * ih);
    }
    b.e2x = -(ud[2] * b.e1y);
    b.e2y = ud[2] * b.e1x;
    b.e2z = fm(ud[0], b.e1y, -(ud[1] * b.e1x));
    b.k1 = -fm(o[1], b.e1y, o[0] * b.e1x);
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
// rayz_hip.hip: pad_radius2_scan, pad_radius2_bucket, pad_radius2_set
static float pad_r2(const double* s, double S, bool f64_rays, double h, double radius) {
    const double E = (f64_rays ? 40.0 : 32.0) * 5.9604644775390625e-08 * (norm3(s) + norm3(s + 3) + h + radius + S);
    const double rp = radius + E;
    return round_up32(rp * rp);
}

// flat_scan.hpp: plane_run_k1 / _k2, bucket_k1 / _k2, then PackedGroup::discs of the xy basis on a block without cy and vy
static void set_k(const Basis& b, bool movy, float v0, float cy, float ft, float& K1, float& K2) {
    K1 = fm(cy, b.e1y, b.k1), K2 = fm(cy, b.e2y, b.k2);
    if (movy) K1 = fm(v0, ft * b.e1y, K1), K2 = fm(v0, ft * b.e2y, K2);
}
static float plane_disc(const Basis& b, float K1, float K2, float cx, float cz, float r2) {
    const float p1 = fm(cx, b.e1x, K1);
    float p2 = fm(cx, b.e2x, K2);
    p2 = fm(cz, b.e2z, p2);
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
        float out[10];
        set_k(b, a[19] != 0, (float)a[17], (float)a[16], (float)a[26], out[8], out[9]);
        for (int k = 0; k < 8; ++k) out[k] = plane_disc(b, out[8], out[9], (float)a[k], (float)a[8 + k], (float)a[36]);
        std::fwrite(out, sizeof(float), 10, stdout);
    }
    return 0;
}

struct ClassLayout {
    std::vector<rayz_plane::PlaneRun> runs;
    std::vector<std::vector<uint32_t>> members, parent_order; // slot order with and without sets
    std::vector<rayz_plane::RunBuckets> buckets;
    std::vector<rayz_plane::ClassSet> sets;
    std::vector<uint32_t> run_old_first, bucket_old_first;
    uint32_t plane_slots = 0;
};

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string cmd = argv[1];
    if (cmd == "discs") return argc < 4 ? 2 : discs(argv[2], std::atoi(argv[3]) != 0);
    const std::vector<double> sph = read_rows(argv[2]);
    const size_t ns = sph.size() / 7;
    std::vector<uint32_t> cls[2];
    for (uint32_t i = 0; i < ns; ++i) {
        const double* s = &sph[7 * i];
        if (s[3] == 0 && s[5] == 0) cls[s[4] != 0].push_back(i); // rayz_hip.hip: velocity_class
    }
    auto cy_of = [&](uint32_t pool) { return (float)sph[7 * pool + 1]; };
    auto vy_of = [&](uint32_t pool) { return (float)sph[7 * pool + 4]; };
    auto vy64_of = [&](uint32_t pool) { return sph[7 * pool + 4]; };
    auto r_of = [&](uint32_t pool) { return std::fabs(sph[7 * pool + 6]); };
    ClassLayout L[2];
    for (int c = 0; c < 2; ++c) { // rayz_hip.hip: plan_slots
        std::vector<uint32_t> loose;
        L[c].plane_slots = rayz_plane::plan_runs(cls[c], cy_of, 4, L[c].runs, L[c].members, loose);
        if (c == 1)
            for (std::vector<uint32_t>& m : L[c].members) {
                L[c].buckets.push_back(rayz_plane::plan_buckets(m, vy_of, r_of, 4));
                m = L[c].buckets.back().order;
            }
        L[c].parent_order = L[c].members;
        rayz_plane::plan_class_sets(L[c].runs, L[c].members, c == 1 ? &L[c].buckets : nullptr, r_of, vy64_of, L[c].sets, L[c].run_old_first,
                                    L[c].bucket_old_first);
    }
    if (cmd == "layout") {
        std::printf("{\"iter\": %u, \"classes\": [", rayz_plane::kSetIter);
        for (int c = 0; c < 2; ++c) {
            std::printf("%s{\"plane_slots\": %u, \"runs\": [", c ? ", " : "", L[c].plane_slots);
            for (size_t j = 0, b = 0; j < L[c].runs.size(); ++j) {
                std::printf("%s{\"first\": %u, \"end\": %u, \"old_first\": %u, \"order\": [", j ? ", " : "", L[c].runs[j].first, L[c].runs[j].end,
                            L[c].run_old_first[j]);
                for (size_t k = 0; k < L[c].members[j].size(); ++k) std::printf("%s%u", k ? ", " : "", L[c].members[j][k]);
                std::printf("], \"parent_order\": [");
                for (size_t k = 0; k < L[c].parent_order[j].size(); ++k) std::printf("%s%u", k ? ", " : "", L[c].parent_order[j][k]);
                std::printf("], \"buckets\": [");
                uint32_t at = L[c].runs[j].first;
                for (size_t q = 0; c == 1 && q < L[c].buckets[j].count.size(); ++q, ++b) {
                    std::printf("%s{\"first\": %u, \"end\": %u, \"old_first\": %u, \"v0_bits\": %u}", q ? ", " : "", at, at + L[c].buckets[j].count[q],
                                L[c].bucket_old_first[b], rayz_plane::bits32(L[c].buckets[j].v0[q]));
                    at += L[c].buckets[j].count[q];
                }
                std::printf("]}");
            }
            std::printf("], \"sets\": [");
            for (size_t k = 0; k < L[c].sets.size(); ++k) {
                const rayz_plane::ClassSet& t = L[c].sets[k];
                std::printf("%s{\"run\": %u, \"bucket\": %d, \"first\": %u, \"end\": %u, \"Rp\": %.17g, \"v0_bits\": %u}", k ? ", " : "", t.run, t.bucket,
                            t.first, t.first + t.count, t.Rp, rayz_plane::bits32(t.v0));
            }
            std::printf("]}");
        }
        std::printf("]}\n");
        return 0;
    }
    if (cmd != "audit" || argc < 6) return 2;
    const std::vector<double> rays = read_rows(argv[3]);
    const double S = std::atof(argv[4]);
    const bool f64_rays = std::atoi(argv[5]) != 0;
    unsigned long long pairs = 0, hits = 0, cands = 0, xy = 0, fneg = 0, lost = 0;
    double ratio = 0, min_ratio = INFINITY, member_ratio = 0, pad_spread = 0;
    auto center_of = [&](uint32_t pool) { return &sph[7 * pool]; };
    auto velocity_of = [&](uint32_t pool) { return &sph[7 * pool + 3]; };
    for (int c = 0; c < 2; ++c)
        for (const rayz_plane::ClassSet& t : L[c].sets) {
            const rayz_plane::PlaneRun& run = L[c].runs[t.run];
            // R2: the library's own, what the set's record in the stream holds (rayz_hip.hip: append_sets calls the same function on
            // the same layout); own[k]: the padded square the member's XY form holds, restated here
            const float R2 = rayz_plane::class_set_r2(t, run, L[c].members[t.run], center_of, velocity_of, S, f64_rays);
            std::vector<float> own(t.count);
            double e_min = INFINITY, e_max = 0, key_min = INFINITY;
            for (uint32_t k = 0; k < t.count; ++k) {
                const double* s = &sph[7 * L[c].members[t.run][t.first - run.first + k]];
                const double h = c == 1 ? rayz_plane::bucket_h(s[4], t.v0) : 0.0;
                own[k] = pad_r2(s, S, f64_rays, h, std::fabs(s[6]) + h); // pad_radius2_bucket (= pad_radius2_scan at h = 0)
                const double mine = pad_r2(s, S, f64_rays, h, t.Rp), e = std::sqrt((double)mine) - t.Rp; // the member as the sphere of radius R'
                member_ratio = std::max(member_ratio, std::sqrt((double)mine / (double)own[k]));
                e_min = std::min(e_min, e), e_max = std::max(e_max, e), key_min = std::min(key_min, std::fabs(s[6]) + h);
            }
            pad_spread = std::max(pad_spread, (e_max - e_min) / key_min); // R2 is the LARGEST member's: the others carry its pad
            for (uint32_t k = 0; k < t.count; ++k) {
                ratio = std::max(ratio, std::sqrt((double)R2 / (double)own[k]));
                min_ratio = std::min(min_ratio, (double)R2 / (double)own[k]);
            }
            for (size_t i = 0; i + 7 <= rays.size(); i += 7) {
                const double* ry = &rays[i];
                const Basis b = ray_basis(ry, ry + 3, f64_rays);
                float K1, K2;
                set_k(b, c == 1, t.v0, run.cy, (float)ry[6], K1, K2);
                for (uint32_t k = 0; k < t.count; ++k) {
                    const double* s = &sph[7 * L[c].members[t.run][t.first - run.first + k]];
                    const bool cand = plane_disc(b, K1, K2, (float)s[0], (float)s[2], R2) >= 0.0f;
                    const bool was = plane_disc(b, K1, K2, (float)s[0], (float)s[2], own[k]) >= 0.0f;
                    const bool hit = f64_hit(s, ry, f64_rays);
                    ++pairs, hits += hit, cands += cand, xy += was, fneg += hit && !cand, lost += was && !cand;
                }
            }
        }
    std::printf("{\"pairs\": %llu, \"f64_hits\": %llu, \"candidates\": %llu, \"xy_candidates\": %llu, \"false_negatives\": %llu, "
                "\"lost\": %llu, \"max_radius_ratio\": %.17g, \"min_r2_over_own\": %.17g, \"max_member_ratio\": %.17g, \"max_pad_spread\": %.17g}\n",
                pairs, hits, cands, xy, fneg, lost, ratio, min_ratio, member_ratio, pad_spread);
    return 0;
}
