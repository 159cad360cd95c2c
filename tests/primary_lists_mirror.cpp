// primary_lists_mirror.cpp — the library's own beam test (rayz_amd/csrc/primary_lists.hpp) on the CPU, for
// tests/test_primary_lists_cpu.py.  Spheres: rows of 7 doubles {c, v, r}; the camera: 19 doubles {from, du, dv, pxo, defu, defv,
// defocus}; samples: rows of 7 doubles {px, py, vx, vy, jx, jy, time}.
//   counts  <spheres> <camera> <width> <height>            u32 list length of every pixel (row-major; kNoList beyond kListK) to stdout
//   hist    <spheres> <camera> <width> <height> [stride]   JSON: the histogram of the list lengths
//   check   <spheres> <camera> <samples>                   JSON: every (sample, sphere) pair decided by the f64 quadratic, held to the lists
//   check32 <spheres> <camera> <samples>                   the same for the ray the f32 kernels trace: the camera narrowed to float, o, d and
//                                                          the time formed in float in camera_ray<float>'s operation order (shade.hpp)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../rayz_amd/csrc/primary_lists.hpp"

using namespace rayz_primary;

static std::vector<double> read_doubles(const char* path) {
    std::vector<double> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(2);
    }
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(double));
    if (std::fread(v.data(), sizeof(double), v.size(), f) != v.size()) std::exit(2);
    std::fclose(f);
    return v;
}

static BeamCamera read_camera(const char* path) {
    const std::vector<double> v = read_doubles(path);
    if (v.size() != 19) {
        std::fprintf(stderr, "camera: 19 doubles\n");
        std::exit(2);
    }
    BeamCamera c;
    std::memcpy(c.from, &v[0], 24), std::memcpy(c.du, &v[3], 24), std::memcpy(c.dv, &v[6], 24);
    std::memcpy(c.pxo, &v[9], 24), std::memcpy(c.defu, &v[12], 24), std::memcpy(c.defv, &v[15], 24);
    c.defocus = v[18] != 0.0;
    return c;
}

// The pixel's list as primary_lists_kernel builds it: sphere numbers in order; false when more than kListK pass.
static bool pixel_list(const BeamCamera& cam, const std::vector<double>& sph, uint32_t px, uint32_t py, std::vector<uint32_t>& list,
                       uint32_t& passed) {
    const PixelBeam b = pixel_beam(cam, px, py);
    list.clear();
    passed = 0;
    for (size_t i = 0; i < sph.size() / 7; ++i) {
        const double* s = &sph[7 * i];
        if (beam_may_hit(b, s, s + 3, s[6])) {
            ++passed;
            if (list.size() < kListK) list.push_back((uint32_t)i);
        }
    }
    return passed <= kListK;
}

int main(int argc, char** argv) {
    if (argc < 4) return 2;
    const std::string cmd = argv[1];
    const std::vector<double> sph = read_doubles(argv[2]);
    const BeamCamera cam = read_camera(argv[3]);
    std::vector<uint32_t> list;
    uint32_t passed = 0;
    if ((cmd == "counts" && argc == 6) || (cmd == "hist" && (argc == 6 || argc == 7))) {
        const uint32_t w = (uint32_t)std::atoi(argv[4]), h = (uint32_t)std::atoi(argv[5]);
        const uint32_t stride = argc == 7 ? (uint32_t)std::atoi(argv[6]) : 1u; // hist: every stride-th pixel of every stride-th row
        uint64_t seen = 0;
        std::vector<uint32_t> counts((size_t)w * h);
        std::map<uint32_t, uint64_t> hist;
        uint64_t sum = 0, mx = 0;
        for (uint32_t py = 0; py < h; py += stride)
            for (uint32_t px = 0; px < w; px += stride) {
                ++seen;
                const bool ok = pixel_list(cam, sph, px, py, list, passed);
                counts[(size_t)py * w + px] = ok ? passed : kNoList;
                hist[passed]++;
                sum += passed;
                mx = passed > mx ? passed : mx;
            }
        if (cmd == "counts") {
            std::fwrite(counts.data(), sizeof(uint32_t), counts.size(), stdout);
            return 0;
        }
        std::printf("{\"k\": %u, \"pixels\": %llu, \"mean\": %.4f, \"max\": %llu, \"hist\": {", kListK, (unsigned long long)seen,
                    (double)sum / (double)seen, (unsigned long long)mx);
        bool first = true;
        for (const auto& kv : hist) {
            std::printf("%s\"%u\": %llu", first ? "" : ", ", kv.first, (unsigned long long)kv.second);
            first = false;
        }
        std::printf("}}\n");
        return 0;
    }
    if ((cmd == "check" || cmd == "check32") && argc == 5) {
        const bool f32 = cmd == "check32";
        const std::vector<double> smp = read_doubles(argv[4]);
        const size_t n = smp.size() / 7;
        uint64_t hits = 0, misses = 0, nolist = 0, listed_hits = 0;
        std::string first_miss;
        for (size_t j = 0; j < n; ++j) {
            const double* s = &smp[7 * j];
            const uint32_t px = (uint32_t)s[0], py = (uint32_t)s[1];
            const bool ok = pixel_list(cam, sph, px, py, list, passed);
            nolist += !ok;
            double o[3], d[3];
            for (int k = 0; k < 3; ++k) {
                o[k] = cam.from[k] + (cam.defocus ? cam.defu[k] * s[2] + cam.defv[k] * s[3] : 0.0);
                d[k] = (cam.pxo[k] + cam.du[k] * ((double)px + s[4]) + cam.dv[k] * ((double)py + s[5])) - o[k];
            }
            double time = s[6];
            if (f32) {
                const float x = (float)px + (float)s[4], y = (float)py + (float)s[5], vx = (float)s[2], vy = (float)s[3];
                for (int k = 0; k < 3; ++k) {
                    float of = (float)cam.from[k];
                    if (cam.defocus) of = of + fmaf((float)cam.defv[k], vy, (float)cam.defu[k] * vx);
                    o[k] = of;
                    d[k] = (fmaf((float)cam.dv[k], y, (float)cam.du[k] * x) + (float)cam.pxo[k]) - of;
                }
                time = (float)s[6];
            }
            const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
            for (size_t i = 0; i < sph.size() / 7; ++i) {
                const double* q = &sph[7 * i];
                double e[3];
                for (int k = 0; k < 3; ++k) e[k] = q[k] + q[3 + k] * time - o[k];
                const double hb = d[0] * e[0] + d[1] * e[1] + d[2] * e[2];
                const double cc = e[0] * e[0] + e[1] * e[1] + e[2] * e[2] - q[6] * q[6];
                const double disc = hb * hb - a * cc;
                if (!(disc >= 0.0) || !((hb + std::sqrt(disc)) / a > 0.0)) continue; // no root at t > 0
                ++hits;
                if (!ok) continue; // a "no list" pixel scans
                bool in = false;
                for (uint32_t x : list) in = in || x == (uint32_t)i;
                listed_hits += in;
                if (!in) {
                    if (!misses) first_miss = "[" + std::to_string(j) + ", " + std::to_string(i) + "]";
                    ++misses;
                }
            }
        }
        std::printf("{\"samples\": %zu, \"hits\": %llu, \"listed_hits\": %llu, \"misses\": %llu, \"nolist_samples\": %llu, \"first_miss\": %s}\n", n,
                    (unsigned long long)hits, (unsigned long long)listed_hits, (unsigned long long)misses, (unsigned long long)nolist,
                    misses ? first_miss.c_str() : "null");
        return 0;
    }
    return 2;
}
