// A plain C++ restatement of the variance-guided à-trous filter, DESIGN.md §4.13, written from that section; it includes no library
// header.  Built by tests/denoise_guided_ref.py with `g++ -O2 -ffp-contract=off` as a shared object, as tests/denoise_mirror.cpp is;
// it is held, independently of the device, to the hand-derived answers of tests/denoise_guided_cases.py, and the GPU tests hold
// the device to it bit for bit.
//
// §4.13 in short.  Everything of §4.11 stands (m, e, h, g = wn·wz, the skipped background-versus-hit tap, j outer and i inner,
// every tap reads the level's input); the colour weight changes and a variance channel v rides along.
//   Pack:  t = ((var_r / (m_r·m_r)) + (var_g / (m_g·m_g))) + (var_b / (m_b·m_b));  v = !(t < VCAP) ? VCAP : (t > 0 ? t : 0);  VCAP = 2^32.
//   Level, pixel p.  Prefilter: taps q = p + (i, j), i, j in -1..1 at distance 1 whatever the stride, j outer, i inner; a tap
//     outside the frame or with bg(q) != bg(p) is skipped; gg = gk[i]·gk[j], gk = {1/4, 1/2, 1/4};  G = G + gg;  A = fma(gg, v_q, A);
//     gv = A / G.
//   Then for every one of the 25 taps §4.11 accepts:
//     den = sc2·(gv + vf);  wc = 1 / (1 + de2 / den);  w = (h·g)·wc;
//     W = W + w;  S_ch = fma(w, e_q.ch, S_ch);  V = fma(w·w, v_q, V)
//   Output of the level: colour S_ch / W, variance V / (W·W).
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace {

inline float dot3(const float* a, const float* b) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }
inline float max0(float x) { return x > 0.0f ? x : 0.0f; }
const float K[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
const float GK[3] = {0.25f, 0.5f, 0.25f};
const float VCAP = 4294967296.0f;

} // namespace

extern "C" {

// Records, 4 floats per pixel each: ga = {n, bg ? 1 : 0}, gb = {P, 0}, mod = {m, 0}, col = {e, v}.
void denoise_guided_mirror_pack(const float* rgb, const float* var_rgb, const int32_t* index, const float* normal, const float* point,
                                const float* albedo_or_null, float* ga, float* gb, float* mod, float* col, size_t n) {
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
        const float tr = var_rgb[3 * p] / (m[0] * m[0]), tg = var_rgb[3 * p + 1] / (m[1] * m[1]), tb = var_rgb[3 * p + 2] / (m[2] * m[2]);
        const float t = (tr + tg) + tb;
        ga[4 * p + 3] = bg ? 1.0f : 0.0f;
        gb[4 * p + 3] = mod[4 * p + 3] = 0.0f;
        col[4 * p + 3] = !(t < VCAP) ? VCAP : (t > 0.0f ? t : 0.0f);
    }
}

// Rows [y0, y1) of level l: src -> dst (4 floats per pixel: colour and variance).
void denoise_guided_mirror_level(const float* ga, const float* gb, const float* src, float* dst, uint32_t width, uint32_t height,
                                 uint32_t l, uint32_t normal_power_log2, float sp2, float sc2, float vf, uint32_t y0, uint32_t y1) {
    const long s = 1l << l;
    for (long y = y0; y < (long)y1; ++y)
        for (long x = 0; x < (long)width; ++x) {
            const size_t p = (size_t)y * width + x;
            const float *np = ga + 4 * p, *Pp = gb + 4 * p, *ep = src + 4 * p;
            const bool bgp = np[3] != 0.0f;
            float G = 0.0f, A = 0.0f;
            for (int j = -1; j <= 1; ++j)
                for (int i = -1; i <= 1; ++i) {
                    const long qx = x + i, qy = y + j;
                    if (qx < 0 || qx >= (long)width || qy < 0 || qy >= (long)height) continue;
                    const size_t q = (size_t)qy * width + qx;
                    if ((ga[4 * q + 3] != 0.0f) != bgp) continue;
                    const float gg = GK[i + 1] * GK[j + 1];
                    G = G + gg;
                    A = std::fmaf(gg, src[4 * q + 3], A);
                }
            const float gv = A / G;
            const float den = sc2 * (gv + vf);
            float W = 0.0f, S[3] = {0.0f, 0.0f, 0.0f}, V = 0.0f;
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
                    const float wc = 1.0f / (1.0f + dot3(de, de) / den);
                    const float w = (h * g) * wc;
                    W = W + w;
                    for (int c = 0; c < 3; ++c) S[c] = std::fmaf(w, eq[c], S[c]);
                    V = std::fmaf(w * w, eq[3], V);
                }
            for (int c = 0; c < 3; ++c) dst[4 * p + c] = S[c] / W;
            dst[4 * p + 3] = V / (W * W);
        }
}

// After the last level: packed RGB = e x m; the variance as the level left it.
void denoise_guided_mirror_finish(const float* col, const float* mod, float* rgb, float* var, size_t n) {
    for (size_t p = 0; p < n; ++p) {
        for (int c = 0; c < 3; ++c) rgb[3 * p + c] = col[4 * p + c] * mod[4 * p + c];
        var[p] = col[4 * p + 3];
    }
}

} // extern "C"
