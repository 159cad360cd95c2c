// CPU mirror of the flat list's plane-run layout and of its plane-form reject test (tests/test_plane_runs.py).
// Built by the test with g++ -ffp-contract=off: every fm() below is one std::fma, as on the GPU.
//   layout <spheres>               -> the plane runs of the static and mov-Y classes (rayz_plane::plan_runs)
//   audit <spheres> <rays> <S> <f64>  -> the plane-form f32 filter against the f64 discriminant for every (ray, sphere) pair
//   pairs <spheres> <rays> <S> <f64>  -> the same for ray i against sphere i only
//   discs <records> <f64>          -> per RAYZ_KAT_SCAN_DISCS record of class 2 / 3 (a plane run: the run's height cy[4]), the
//                                     plane-form value of its four spheres and the value of a pad slot (r² = -inf) at their
//                                     place: 8 raw f32 on stdout.  The record carries the library's padded r² at [28..31].
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

// the kernel's unit(d) in R (device_math.hpp: dot3, sq, 1/m, products)
template <class R> static void unit(const double* d, R* u) {
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

// rayz_hip.hip: pad_radius2_scan (E = 32u or 40u (|c| + |v| + r + S), squared in f64, rounded up to f32)
static float pad_r2(const double* s, double S, bool f64_rays) {
    const double u = 5.9604644775390625e-08;
    const double E = (f64_rays ? 40.0 : 32.0) * u *
                     (std::sqrt(s[0] * s[0] + s[1] * s[1] + s[2] * s[2]) + std::sqrt(s[3] * s[3] + s[4] * s[4] + s[5] * s[5]) +
                      std::fabs(s[6]) + S);
    const double rp = std::fabs(s[6]) + E, v = rp * rp;
    float f = (float)v;
    if ((double)f < v) f = std::nextafter(f, INFINITY);
    return f;
}

// The plane form of a block as the device runs it for a plane run (flat_scan.hpp: scan_plane_class puts K2 in the basis,
// ScanGroup<float, 3 / 4>::discs), from a KAT record: the ray as kat_kernel narrows it (unit(d) in R, then f32).
static int discs(const char* path, bool f64_rays) {
    const std::vector<double> rec = read_rows(path);
    for (size_t i = 0; i + 48 <= rec.size(); i += 48) {
        const double* a = &rec[i];
        if (a[27] != 2.0 && a[27] != 3.0) return 3;
        float ud[3];
        if (f64_rays) {
            double u64[3];
            unit<double>(a + 23, u64);
            for (int j = 0; j < 3; ++j) ud[j] = (float)u64[j];
        } else {
            unit<float>(a + 23, ud);
        }
        const float o[3] = {(float)a[20], (float)a[21], (float)a[22]}, ft = (float)a[26];
        const Basis b = make_basis(ud, o);
        const float K2 = fm((float)a[4], b.e2y, b.k2);
        float out[8];
        for (int k = 0; k < 4; ++k) {
            const float cx = (float)a[k], cz = (float)a[8 + k], vy = (float)a[16 + k];
            float p1 = fm(cx, b.e1x, b.k1), p2 = fm(cx, b.e2x, K2);
            p1 = fm(cz, b.e1z, p1);
            p2 = fm(cz, b.e2z, p2);
            if (a[27] == 3.0) p2 = fm(vy, ft * b.e2y, p2);
            out[k] = fm(-p1, p1, fm(-p2, p2, (float)a[28 + k]));
            out[4 + k] = fm(-p1, p1, fm(-p2, p2, -INFINITY));
        }
        std::fwrite(out, sizeof(float), 8, stdout);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    if (std::string(argv[1]) == "discs") return argc < 4 ? 2 : discs(argv[2], std::atoi(argv[3]) != 0);
    const std::vector<double> sph = read_rows(argv[2]);
    const size_t ns = sph.size() / 7;
    std::vector<uint32_t> cls[2];
    std::vector<int> cls_of(ns, 2);
    for (uint32_t i = 0; i < ns; ++i) {
        const double* s = &sph[7 * i];
        if (s[3] == 0 && s[5] == 0) cls_of[i] = s[4] == 0 ? 0 : 1, cls[cls_of[i]].push_back(i); // static / mov-Y (velocity_class)
    }
    auto cy_of = [&](uint32_t pool) { return (float)sph[7 * pool + 1]; };
    if (std::string(argv[1]) == "layout") {
        std::printf("{\"group\": %d, \"classes\": [", 4);
        for (int c = 0; c < 2; ++c) {
            std::vector<rayz_plane::PlaneRun> runs;
            std::vector<std::vector<uint32_t>> members;
            std::vector<uint32_t> loose;
            const uint32_t slots = rayz_plane::plan_runs(cls[c], cy_of, 4, runs, members, loose);
            std::printf("%s{\"n\": %zu, \"plane_slots\": %u, \"runs\": [", c ? ", " : "", cls[c].size(), slots);
            for (size_t j = 0; j < runs.size(); ++j) {
                std::printf("%s{\"cy\": %.9g, \"first\": %u, \"end\": %u, \"members\": [", j ? ", " : "", runs[j].cy, runs[j].first, runs[j].end);
                for (size_t k = 0; k < members[j].size(); ++k) std::printf("%s%u", k ? ", " : "", members[j][k]);
                std::printf("]}");
            }
            std::printf("], \"loose\": [");
            for (size_t k = 0; k < loose.size(); ++k) std::printf("%s%u", k ? ", " : "", loose[k]);
            std::printf("]}");
        }
        std::printf("]}\n");
        return 0;
    }
    if (argc < 6) return 2;
    const std::vector<double> rays = read_rows(argv[3]);
    const double S = std::atof(argv[4]);
    const bool f64_rays = std::atoi(argv[5]) != 0, diagonal = std::string(argv[1]) == "pairs";
    unsigned long long pairs = 0, hits = 0, cands = 0, fneg = 0, pad_pass = 0;
    std::vector<float> r2(ns);
    for (size_t i = 0; i < ns; ++i) r2[i] = pad_r2(&sph[7 * i], S, f64_rays);
    for (size_t k = 0; k + 7 <= rays.size(); k += 7) {
        const double* ry = &rays[k];
        float ud[3];
        if (f64_rays) { // the f64 kernel: unit(d) in f64, then the ray narrowed to f32 for the filter
            double u64[3];
            unit<double>(ry + 3, u64);
            for (int j = 0; j < 3; ++j) ud[j] = (float)u64[j];
        } else {
            unit<float>(ry + 3, ud);
        }
        const float o[3] = {(float)ry[0], (float)ry[1], (float)ry[2]}, ft = (float)ry[6];
        const Basis b = make_basis(ud, o);
        const double ox = f64_rays ? ry[0] : (double)o[0], oy = f64_rays ? ry[1] : (double)o[1], oz = f64_rays ? ry[2] : (double)o[2];
        const double dx = f64_rays ? ry[3] : (double)(float)ry[3], dy = f64_rays ? ry[4] : (double)(float)ry[4],
                     dz = f64_rays ? ry[5] : (double)(float)ry[5], tt = f64_rays ? ry[6] : (double)ft;
        const double a = fm(dz, dz, fm(dy, dy, dx * dx));
        std::vector<uint32_t> own;
        if (diagonal && k / 7 < ns && cls_of[k / 7] < 2) own.push_back((uint32_t)(k / 7));
        for (int c = 0; c < 2; ++c)
            for (uint32_t pool : diagonal ? own : cls[c]) {
                if (cls_of[pool] != c) continue;
                const double* s = &sph[7 * pool];
                // the plane form (flat_scan.hpp: ScanGroup<float, 3 / 4>::discs), the sphere's own f32 cy as the run's
                const float cx = (float)s[0], cy = (float)s[1], cz = (float)s[2], vy = (float)s[4];
                const float K2 = fm(cy, b.e2y, b.k2);
                float p1 = fm(cx, b.e1x, b.k1), p2 = fm(cx, b.e2x, K2);
                p1 = fm(cz, b.e1z, p1);
                p2 = fm(cz, b.e2z, p2);
                if (c == 1) p2 = fm(vy, ft * b.e2y, p2);
                const bool cand = fm(-p1, p1, fm(-p2, p2, r2[pool])) >= 0.0f;
                if (fm(-p1, p1, fm(-p2, p2, -INFINITY)) >= 0.0f) ++pad_pass; // a pad slot of the same run
                // the narrow phase's f64 discriminant (flat_scan.hpp: narrow_eval) on the pool's f64 sphere
                const double qx = fm(s[3], tt, s[0] - ox), qy = fm(s[4], tt, s[1] - oy), qz = fm(s[5], tt, s[2] - oz);
                const double hb = fm(dz, qz, fm(dy, qy, dx * qx));
                const double cc = fm(qz, qz, fm(qy, qy, fm(qx, qx, -(s[6] * s[6]))));
                const bool hit = fm(-a, cc, hb * hb) >= 0.0;
                ++pairs, hits += hit, cands += cand, fneg += hit && !cand;
            }
    }
    std::printf("{\"pairs\": %llu, \"f64_hits\": %llu, \"candidates\": %llu, \"false_negatives\": %llu, \"pad_passes\": %llu}\n",
                pairs, hits, cands, fneg, pad_pass);
    return 0;
}
