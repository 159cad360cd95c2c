// A plain C++ restatement of the à-trous denoiser's arithmetic contract; it includes no library header.  §4.11
// fixes the order of every operation, so a restatement of it necessarily has the shape of the device's dn_tap: what makes it a check
// and not a copy is that it is held, independently of the device, to the hand-derived known answers of tests/test_denoise_cpu.py: the
// 0-or-1-weight answers there, the exact rational cases of tests/denoise_cases.py (proper-fraction wn, wz and wc, worked out in
// Fractions and rounded once) and, on general guides, a float64 statement of §4.11 written from its text (tests/denoise_f64.py)
// within a derived rounding bound that every listed misreading of §4.11 exceeds.
// Built by tests/denoise_ref.py with `g++ -O2 -ffp-contract=off` (so the compiler fuses nothing: an FMA happens exactly where fmaf is written) as a shared object; the tests hold the GPU to it bit for bit.
//
// §4.11 in short.  Per pixel: radiance c, index, unit normal n, point P, albedo a; bg := index < 0.
//   m = demodulate && !bg ? max(a, 2^-8) per channel : 1;   e = c / m;   result = (last level's output) x m.
//   Level l = 0..L-1, stride s = 2^l, taps q = p + s·(i, j), j outer, i inner, both ascending -2..2, taps outside the frame skipped:
//     h  = k[i]·k[j],  k = {1/16, 1/4, 3/8, 1/4, 1/16}
//     if bg(p) or bg(q): the tap counts with g = 1 when both are background and is SKIPPED otherwise
//     else  wn = max(0, dot(n_p, n_q)), then wn = wn·wn, normal_power_log2 times
//           v = P_q - P_p;  d2 = dot(v, v);  pl = dot(n_p, v)
//           wz = d2 == 0 ? 1 : u·u with u = max(0, 1 - (pl·pl) / (sp2·d2))
//           g = wn·wz
//     de = e_q - e_p;  wc = 1 / (1 + (dot(de, de)·4^l) / sc2)
//     w = (h·g)·wc;  W = W + w;  S_ch = fma(w, e_q.ch, S_ch)
//   output of the level: S_ch / W.
//   dot(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x·b.x));  max(0, x) = x > 0 ? x : 0;  max(a, 2^-8) = a > 2^-8 ? a : 2^-8;
//   sp2 = f32(sigma_plane)·f32(sigma_plane), sc2 likewise, both products in f32.
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace {

inline float dot3(const float* a, const float* b) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }
inline float max0(float x) { return x > 0.0f ? x : 0.0f; }
const float K[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};

} // namespace

extern "C" {

// Records, 4 floats per pixel each: ga = {n, bg ? 1 : 0}, gb = {P, 0}, mod = {m, 0}, col = {e, 0}.
void denoise_mirror_pack(const float* rgb, const int32_t* index, const float* normal, const float* point, const float* albedo_or_null,
                         float* ga, float* gb, float* mod, float* col, size_t n) {
    const float lo = 0.00390625f;
    for (size_t p = 0; p < n; ++p) {
        const bool bg = index[p] < 0;
        float m[3] = {1.0f, 1.0f, 1.0f};
        if (albedo_or_null && !bg)
            for (int c = 0; c < 3; ++c) m[c] = albedo_or_null[3 * p + c] > lo ? albedo_or_null[3 * p + c] : lo;
        for (int c = 0; c < 3; ++c) {
            ga[4 * p + c] = normal[3 * p + c];
            gb[4 * p + c] = point[3 * p + c];
            mod[4 * p + c] = m[c];
            col[4 * p + c] = rgb[3 * p + c] / m[c];
        }
        ga[4 * p + 3] = bg ? 1.0f : 0.0f;
        gb[4 * p + 3] = mod[4 * p + 3] = col[4 * p + 3] = 0.0f;
    }
}

// Rows [y0, y1) of level l: src -> dst (4 floats per pixel).
void denoise_mirror_level(const float* ga, const float* gb, const float* src, float* dst, uint32_t width, uint32_t height, uint32_t l,
                          uint32_t normal_power_log2, float sp2, float sc2, uint32_t y0, uint32_t y1) {
    const long s = 1l << l;
    const float cl = (float)(1u << (2 * l));
    for (long y = y0; y < (long)y1; ++y)
        for (long x = 0; x < (long)width; ++x) {
            const size_t p = (size_t)y * width + x;
            const float *np = ga + 4 * p, *Pp = gb + 4 * p, *ep = src + 4 * p;
            const bool bgp = np[3] != 0.0f;
            float W = 0.0f, S[3] = {0.0f, 0.0f, 0.0f};
            for (int j = -2; j <= 2; ++j)
                for (int i = -2; i <= 2; ++i) {
                    const long qx = x + s * i, qy = y + s * j;
                    if (qx < 0 || qx >= (long)width || qy < 0 || qy >= (long)height) continue;
                    const size_t q = (size_t)qy * width + qx;
                    const float *nq = ga + 4 * q, *Pq = gb + 4 * q, *eq = src + 4 * q;
                    const bool bgq = nq[3] != 0.0f;
                    const float h = K[i + 2] * K[j + 2];
                    float g;
                    if (bgp || bgq) {
                        if (!(bgp && bgq)) continue;
                        g = 1.0f;
                    } else {
                        float wn = max0(dot3(np, nq));
                        for (uint32_t k = 0; k < normal_power_log2; ++k) wn = wn * wn;
                        const float v[3] = {Pq[0] - Pp[0], Pq[1] - Pp[1], Pq[2] - Pp[2]};
                        const float d2 = dot3(v, v), pl = dot3(np, v);
                        float wz = 1.0f;
                        if (d2 != 0.0f) {
                            const float u = max0(1.0f - (pl * pl) / (sp2 * d2));
                            wz = u * u;
                        }
                        g = wn * wz;
                    }
                    const float de[3] = {eq[0] - ep[0], eq[1] - ep[1], eq[2] - ep[2]};
                    const float wc = 1.0f / (1.0f + (dot3(de, de) * cl) / sc2);
                    const float w = (h * g) * wc;
                    W = W + w;
                    for (int c = 0; c < 3; ++c) S[c] = std::fmaf(w, eq[c], S[c]);
                }
            for (int c = 0; c < 3; ++c) dst[4 * p + c] = S[c] / W;
            dst[4 * p + 3] = 0.0f;
        }
}

// The re-modulation after the last level: packed RGB = e x m.
void denoise_mirror_finish(const float* col, const float* mod, float* rgb, size_t n) {
    for (size_t p = 0; p < n; ++p)
        for (int c = 0; c < 3; ++c) rgb[3 * p + c] = col[4 * p + c] * mod[4 * p + c];
}

} // extern "C"
