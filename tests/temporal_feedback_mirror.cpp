// A plain C++ restatement of temporal accumulation's feedback mode, DESIGN.md §4.17 (the step, which is §4.16's with the raw first
// moment m1 beside the colour, and the feedback write), written from those sections; it includes no library header and shares no
// code with tests/temporal_moments_mirror.cpp, which the tests hold it against where no feedback is given.  Built by
// tests/temporal_feedback_ref.py with `g++ -O2 -ffp-contract=off` as a shared object; it is held, independently of the device, to
// the hand-derived answers of tests/temporal_feedback_cases.py, and the GPU tests hold the device to it bit for bit.  The host
// part of a step (the camera's matrix) is §4.15's and comes from tests/temporal_mirror.cpp through tests/temporal_ref.py.
//
// §4.17 in short.  A history buffer is five arrays of 4 floats per pixel: hc = {c, N}, h1 = {m1, 0}, hg = {n, bits(index)},
// hp = {P, 0}, hm = {m2, W2}.  The step: taps, acceptance, B, al, k, c_out, N_out, m2, W2 as §4.16; over the accepted taps also
// M1 = fma(b, m1_q, M1) in tap order; with history m1 = fma(al, c − M1/B, M1/B), without m1 = c;
// vt = clamp(max(m2 − m1·m1, 0)·W2 / (1 − W2)); the spatial estimate and the selection as §4.16; h1 receives m1.
// The write: per pixel, if all three channels of the image are finite, {hc.r, hc.g, hc.b} = the image's pixel; nothing else changes.
//
// `variant` selects a NAMED MISREADING of the section (0: the section itself); each must fail a hand-derived case:
//   1 the variance from the returned (possibly fed-back) colour     2 the write also overwrites m1     3 the write overwrites N
//   4 (the older side: tests/temporal_feedback_ref.py's, it chooses the buffers)     5 m1 from the pixel's own record, not the taps
//   6 a non-finite feedback pixel is stored
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace {

inline float dot3(const float* a, const float* b) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }
const float VCAP = 4294967296.0f;
const float BMIN = 0.015625f; // 2^-6
inline float clampv(float t) { return !(t < VCAP) ? VCAP : (t > 0.0f ? t : 0.0f); }

struct Acc {
    float B, H[3], HN, Q[3], HW, M1[3];
};

} // namespace

extern "C" {

// One step.  prev_*: the history the previous step wrote, its colour possibly replaced since (ignored when !has_history);
// next_*: the history this step writes.  is_static: 0 = project with M / from (the PREVIOUS camera's), 1 = the one tap q = p.
void temporal_feedback_mirror_step(const float* rgb, const int32_t* index, const float* normal, const float* point, const float* prev_c,
                                   const float* prev_1, const float* prev_g, const float* prev_p, const float* prev_m, float* next_c,
                                   float* next_1, float* next_g, float* next_p, float* next_m, float* rgb_out, float* var_out,
                                   float* len_out, float* w2_out, uint32_t width, uint32_t height, int has_history, int is_static,
                                   const float* M, const float* from, float spp, float am, float nm, float cm, float r2, float wm,
                                   float mt, int variant) {
    const float Wf = (float)width, Hf = (float)height;
    for (long py = 0; py < (long)height; ++py)
        for (long px = 0; px < (long)width; ++px) {
            const size_t p = (size_t)py * width + px;
            const float c[3] = {rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]};
            const int32_t id = index[p];
            const float* n = normal + 3 * p;
            const float* P = point + 3 * p;
            float co[3] = {c[0], c[1], c[2]}, m1[3] = {c[0], c[1], c[2]}, m2[3] = {c[0] * c[0], c[1] * c[1], c[2] * c[2]}, No = spp, W2 = 1.0f;
            if (id >= 0 && has_history) {
                float w[3];
                for (int j = 0; j < 3; ++j) w[j] = P[j] - from[j];
                const float lim = r2 * dot3(w, w);
                Acc acc{0.0f, {0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 0.0f}, 0.0f, {0.0f, 0.0f, 0.0f}};
                auto tap = [&](long qx, long qy, float b) {
                    if (qx < 0 || qx >= (long)width || qy < 0 || qy >= (long)height) return;
                    const size_t q = (size_t)qy * width + qx;
                    int32_t qid;
                    std::memcpy(&qid, prev_g + 4 * q + 3, 4);
                    if (qid != id) return;
                    if (!(dot3(prev_g + 4 * q, n) >= cm)) return;
                    const float d[3] = {prev_p[4 * q] - P[0], prev_p[4 * q + 1] - P[1], prev_p[4 * q + 2] - P[2]};
                    if (!(dot3(d, d) <= lim)) return;
                    const size_t q1 = variant == 5 ? p : q;
                    acc.B = acc.B + b;
                    for (int ch = 0; ch < 3; ++ch) {
                        acc.H[ch] = std::fmaf(b, prev_c[4 * q + ch], acc.H[ch]);
                        acc.Q[ch] = std::fmaf(b, prev_m[4 * q + ch], acc.Q[ch]);
                        acc.M1[ch] = std::fmaf(b, prev_1[4 * q1 + ch], acc.M1[ch]);
                    }
                    acc.HN = std::fmaf(b, prev_c[4 * q + 3], acc.HN);
                    acc.HW = std::fmaf(b, prev_m[4 * q + 3], acc.HW);
                };
                if (is_static) {
                    tap(px, py, 1.0f);
                } else {
                    const float al = std::fmaf(M[2], w[2], std::fmaf(M[1], w[1], M[0] * w[0]));
                    const float be = std::fmaf(M[5], w[2], std::fmaf(M[4], w[1], M[3] * w[0]));
                    const float ga = std::fmaf(M[8], w[2], std::fmaf(M[7], w[1], M[6] * w[0]));
                    if (ga > 0.0f) {
                        const float x = al / ga, y = be / ga;
                        if (x > -1.0f && x < Wf && y > -1.0f && y < Hf) {
                            const float x0 = std::floor(x), y0 = std::floor(y);
                            const float fx = x - x0, fy = y - y0;
                            for (int j = 0; j < 2; ++j)
                                for (int i = 0; i < 2; ++i)
                                    tap((long)x0 + i, (long)y0 + j, (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy));
                        }
                    }
                }
                if (acc.B >= BMIN) {
                    const float hN = acc.HN / acc.B;
                    const float Ns = hN + spp;
                    const float a0 = spp / Ns;
                    const float a = a0 < am ? am : a0;
                    const float k = 1.0f - a;
                    for (int ch = 0; ch < 3; ++ch) {
                        const float h = acc.H[ch] / acc.B, hq = acc.Q[ch] / acc.B, h1 = acc.M1[ch] / acc.B;
                        co[ch] = std::fmaf(a, c[ch] - h, h);
                        m1[ch] = std::fmaf(a, c[ch] - h1, h1);
                        m2[ch] = std::fmaf(a, c[ch] * c[ch] - hq, hq);
                    }
                    W2 = std::fmaf(k * k, acc.HW / acc.B, a * a);
                    No = Ns > nm ? nm : Ns;
                }
            }
            float vt[3], vs[3] = {VCAP, VCAP, VCAP};
            for (int ch = 0; ch < 3; ++ch) {
                const float mean = variant == 1 ? co[ch] : m1[ch];
                const float e = m2[ch] - (mean * mean);
                const float ep = e > 0.0f ? e : 0.0f;
                vt[ch] = clampv((ep * W2) / (1.0f - W2));
            }
            const bool spatial = id >= 0 && W2 > wm;
            if (spatial) {
                float S0 = 0.0f, S1[3] = {0.0f, 0.0f, 0.0f}, S2[3] = {0.0f, 0.0f, 0.0f};
                for (long j = -3; j <= 3; ++j)
                    for (long i = -3; i <= 3; ++i) {
                        const long qx = px + i, qy = py + j;
                        if (qx < 0 || qx >= (long)width || qy < 0 || qy >= (long)height) continue;
                        const size_t q = (size_t)qy * width + qx;
                        if (index[q] != id) continue;
                        if (!(q == p || dot3(normal + 3 * q, n) >= cm)) continue;
                        S0 = S0 + 1.0f;
                        for (int ch = 0; ch < 3; ++ch) {
                            S1[ch] = S1[ch] + rgb[3 * q + ch];
                            S2[ch] = std::fmaf(rgb[3 * q + ch], rgb[3 * q + ch], S2[ch]);
                        }
                    }
                if (S0 >= mt)
                    for (int ch = 0; ch < 3; ++ch) {
                        const float mu = S1[ch] / S0;
                        const float d = S2[ch] / S0 - mu * mu;
                        const float dp = d > 0.0f ? d : 0.0f;
                        vs[ch] = clampv(((dp * S0) / (S0 - 1.0f)) * W2);
                    }
            }
            for (int ch = 0; ch < 3; ++ch) {
                next_c[4 * p + ch] = rgb_out[3 * p + ch] = co[ch];
                var_out[3 * p + ch] = id < 0 ? 0.0f : (spatial ? vs[ch] : vt[ch]);
                next_1[4 * p + ch] = m1[ch];
                next_g[4 * p + ch] = n[ch];
                next_p[4 * p + ch] = P[ch];
                next_m[4 * p + ch] = m2[ch];
            }
            next_c[4 * p + 3] = No;
            next_1[4 * p + 3] = 0.0f;
            std::memcpy(next_g + 4 * p + 3, &id, 4);
            next_p[4 * p + 3] = 0.0f;
            next_m[4 * p + 3] = W2;
            if (len_out) len_out[p] = No;
            if (w2_out) w2_out[p] = W2;
        }
}

// The feedback write on one history side: hc = {c, N}, h1 = {m1, 0}; image: width·height·3 floats.
void temporal_feedback_mirror_write(float* hc, float* h1, const float* image, uint32_t width, uint32_t height, int variant) {
    const size_t n = (size_t)width * height;
    for (size_t p = 0; p < n; ++p) {
        const float* f = image + 3 * p;
        if (variant != 6 && !(std::isfinite(f[0]) && std::isfinite(f[1]) && std::isfinite(f[2]))) continue;
        for (int ch = 0; ch < 3; ++ch) {
            hc[4 * p + ch] = f[ch];
            if (variant == 2) h1[4 * p + ch] = f[ch];
        }
        if (variant == 3) hc[4 * p + 3] = 0.0f;
    }
}

} // extern "C"
