// A plain C++ restatement of temporal accumulation's counts step, DESIGN.md §4.23 (on §4.15 for the plain handle and on §4.16 for
// the moments handle), written from those sections; it includes no library header.  Built by tests/temporal_counts_ref.py with
// `g++ -O2 -ffp-contract=off` as a shared object, as tests/temporal_mirror.cpp is; it is held, independently of the device, to the
// hand-derived answers of tests/temporal_counts_cases.py and, with uniform counts, to the mirrors of the scalar steps bit for bit;
// the GPU tests hold the device to it bit for bit.  The host part of a step (the camera's matrix) is §4.15's and comes from
// tests/temporal_mirror.cpp through tests/temporal_ref.py.
//
// §4.23 in short.  Per pixel n = f32(count).  A tap is accepted as in §4.15 AND only if its record's length N_q > 0.  No history:
// c_out = c, v_out = s (moments: m2 = c·c, W2 = 1), N_out = n.  History and n > 0: §4.15's step 4 (§4.16's step 2) with n for spp.
// History and n = 0: c_out = h, v_out = hv (moments: m2 = hq, W2 = hW), N_out = min(hN, nm), all by selection — c and s are not
// used.  Moments, step 4: a position of the 7x7 neighbourhood counts only if its own count is > 0, the centre included.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace {

inline float dot3(const float* a, const float* b) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }
const float VCAP = 4294967296.0f;
const float BMIN = 0.015625f; // 2^-6
inline float clampv(float t) { return !(t < VCAP) ? VCAP : (t > 0.0f ? t : 0.0f); }

// What the taps of one pixel sum: B, then per record of four floats the weighted sums.  rec[0] is {c, N}; rec[1] is {v, 0} in the
// plain step and {m2, W2} in the moments step.
struct Sums {
    float B = 0.0f, S[2][4] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
};

struct Frame {
    uint32_t width, height;
    int has_history, is_static;
    const float *M, *from;
    float am, nm, cm, r2;
};

// §4.15 steps 2 and 3 with §4.23's rule 1, for the pixel (px, py) with guides id, n, P.
Sums gather(const Frame& f, long px, long py, int32_t id, const float* n, const float* P, const float* prev_g, const float* prev_p,
            const float* rec0, const float* rec1) {
    Sums acc;
    float w[3];
    for (int j = 0; j < 3; ++j) w[j] = P[j] - f.from[j];
    const float lim = f.r2 * dot3(w, w);
    auto tap = [&](long qx, long qy, float b) {
        if (qx < 0 || qx >= (long)f.width || qy < 0 || qy >= (long)f.height) return;
        const size_t q = (size_t)qy * f.width + qx;
        int32_t qid;
        std::memcpy(&qid, prev_g + 4 * q + 3, 4);
        if (qid != id) return;
        if (!(dot3(prev_g + 4 * q, n) >= f.cm)) return;
        const float d[3] = {prev_p[4 * q] - P[0], prev_p[4 * q + 1] - P[1], prev_p[4 * q + 2] - P[2]};
        if (!(dot3(d, d) <= lim)) return;
        if (!(rec0[4 * q + 3] > 0.0f)) return; // a record of length 0 holds no samples
        acc.B = acc.B + b;
        for (int k = 0; k < 4; ++k) {
            acc.S[0][k] = std::fmaf(b, rec0[4 * q + k], acc.S[0][k]);
            acc.S[1][k] = std::fmaf(b, rec1[4 * q + k], acc.S[1][k]);
        }
    };
    if (f.is_static) {
        tap(px, py, 1.0f);
        return acc;
    }
    const float* M = f.M;
    const float al = std::fmaf(M[2], w[2], std::fmaf(M[1], w[1], M[0] * w[0]));
    const float be = std::fmaf(M[5], w[2], std::fmaf(M[4], w[1], M[3] * w[0]));
    const float ga = std::fmaf(M[8], w[2], std::fmaf(M[7], w[1], M[6] * w[0]));
    if (!(ga > 0.0f)) return acc;
    const float x = al / ga, y = be / ga;
    if (!(x > -1.0f && x < (float)f.width && y > -1.0f && y < (float)f.height)) return acc;
    const float x0 = std::floor(x), y0 = std::floor(y);
    const float fx = x - x0, fy = y - y0;
    for (int j = 0; j < 2; ++j)
        for (int i = 0; i < 2; ++i) tap((long)x0 + i, (long)y0 + j, (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy));
    return acc;
}

} // namespace

extern "C" {

// One counts step of a plain handle.  The arguments are temporal_mirror_step's with `counts` (height·width uint32) for spp.
void temporal_counts_mirror_step(const float* rgb, const float* var, const uint32_t* counts, const int32_t* index, const float* normal,
                                 const float* point, const float* prev_c, const float* prev_v, const float* prev_g, const float* prev_p,
                                 float* next_c, float* next_v, float* next_g, float* next_p, float* rgb_out, float* var_out,
                                 float* len_out, uint32_t width, uint32_t height, int has_history, int is_static, const float* M,
                                 const float* from, float am, float nm, float cm, float r2) {
    const Frame f{width, height, has_history, is_static, M, from, am, nm, cm, r2};
    for (long py = 0; py < (long)height; ++py)
        for (long px = 0; px < (long)width; ++px) {
            const size_t p = (size_t)py * width + px;
            const float* c = rgb + 3 * p;
            const float s[3] = {clampv(var[3 * p]), clampv(var[3 * p + 1]), clampv(var[3 * p + 2])};
            const int32_t id = index[p];
            const float *n = normal + 3 * p, *P = point + 3 * p;
            const float cnt = (float)counts[p];
            float co[3] = {c[0], c[1], c[2]}, vo[3] = {s[0], s[1], s[2]}, No = cnt;
            if (id >= 0 && has_history) {
                const Sums acc = gather(f, px, py, id, n, P, prev_g, prev_p, prev_c, prev_v);
                if (acc.B >= BMIN) {
                    const float hN = acc.S[0][3] / acc.B;
                    if (cnt > 0.0f) {
                        const float Ns = hN + cnt;
                        const float a0 = cnt / Ns;
                        const float a = a0 < am ? am : a0;
                        const float k = 1.0f - a;
                        for (int ch = 0; ch < 3; ++ch) {
                            const float h = acc.S[0][ch] / acc.B, hv = acc.S[1][ch] / acc.B;
                            co[ch] = std::fmaf(a, c[ch] - h, h);
                            vo[ch] = std::fmaf(a * a, s[ch], (k * k) * hv);
                        }
                        No = Ns > nm ? nm : Ns;
                    } else {
                        for (int ch = 0; ch < 3; ++ch) co[ch] = acc.S[0][ch] / acc.B, vo[ch] = acc.S[1][ch] / acc.B;
                        No = hN > nm ? nm : hN;
                    }
                }
            }
            for (int ch = 0; ch < 3; ++ch) {
                next_c[4 * p + ch] = rgb_out[3 * p + ch] = co[ch];
                next_v[4 * p + ch] = var_out[3 * p + ch] = vo[ch];
                next_g[4 * p + ch] = n[ch];
                next_p[4 * p + ch] = P[ch];
            }
            next_c[4 * p + 3] = No;
            next_v[4 * p + 3] = 0.0f;
            std::memcpy(next_g + 4 * p + 3, &id, 4);
            next_p[4 * p + 3] = 0.0f;
            if (len_out) len_out[p] = No;
        }
}

// One counts step of a moments handle.  The arguments are temporal_moments_mirror_step's with `counts` for spp.
void temporal_counts_mirror_step_moments(const float* rgb, const uint32_t* counts, const int32_t* index, const float* normal,
                                         const float* point, const float* prev_c, const float* prev_g, const float* prev_p,
                                         const float* prev_m, float* next_c, float* next_v, float* next_g, float* next_p, float* next_m,
                                         float* rgb_out, float* var_out, float* len_out, float* w2_out, uint32_t width, uint32_t height,
                                         int has_history, int is_static, const float* M, const float* from, float am, float nm,
                                         float cm, float r2, float wm, float mt) {
    const Frame f{width, height, has_history, is_static, M, from, am, nm, cm, r2};
    for (long py = 0; py < (long)height; ++py)
        for (long px = 0; px < (long)width; ++px) {
            const size_t p = (size_t)py * width + px;
            const float* c = rgb + 3 * p;
            const int32_t id = index[p];
            const float *n = normal + 3 * p, *P = point + 3 * p;
            const float cnt = (float)counts[p];
            float co[3] = {c[0], c[1], c[2]}, m2[3] = {c[0] * c[0], c[1] * c[1], c[2] * c[2]}, No = cnt, W2 = 1.0f;
            if (id >= 0 && has_history) {
                const Sums acc = gather(f, px, py, id, n, P, prev_g, prev_p, prev_c, prev_m);
                if (acc.B >= BMIN) {
                    const float hN = acc.S[0][3] / acc.B, hW = acc.S[1][3] / acc.B;
                    if (cnt > 0.0f) {
                        const float Ns = hN + cnt;
                        const float a0 = cnt / Ns;
                        const float a = a0 < am ? am : a0;
                        const float k = 1.0f - a;
                        for (int ch = 0; ch < 3; ++ch) {
                            const float h = acc.S[0][ch] / acc.B, hq = acc.S[1][ch] / acc.B;
                            co[ch] = std::fmaf(a, c[ch] - h, h);
                            m2[ch] = std::fmaf(a, c[ch] * c[ch] - hq, hq);
                        }
                        W2 = std::fmaf(k * k, hW, a * a);
                        No = Ns > nm ? nm : Ns;
                    } else {
                        for (int ch = 0; ch < 3; ++ch) co[ch] = acc.S[0][ch] / acc.B, m2[ch] = acc.S[1][ch] / acc.B;
                        W2 = hW;
                        No = hN > nm ? nm : hN;
                    }
                }
            }
            // §4.16 step 3
            float vt[3], vs[3] = {VCAP, VCAP, VCAP};
            for (int ch = 0; ch < 3; ++ch) {
                const float e = m2[ch] - (co[ch] * co[ch]);
                const float ep = e > 0.0f ? e : 0.0f;
                vt[ch] = clampv((ep * W2) / (1.0f - W2));
            }
            // §4.16 step 4 over the positions that were sampled
            const bool spatial = id >= 0 && W2 > wm;
            if (spatial) {
                float S0 = 0.0f, S1[3] = {0.0f, 0.0f, 0.0f}, S2[3] = {0.0f, 0.0f, 0.0f};
                for (long j = -3; j <= 3; ++j)
                    for (long i = -3; i <= 3; ++i) {
                        const long qx = px + i, qy = py + j;
                        if (qx < 0 || qx >= (long)width || qy < 0 || qy >= (long)height) continue;
                        const size_t q = (size_t)qy * width + qx;
                        if (index[q] != id) continue;
                        if (!(counts[q] > 0)) continue;
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
                const float v = id < 0 ? 0.0f : (spatial ? vs[ch] : vt[ch]);
                next_c[4 * p + ch] = rgb_out[3 * p + ch] = co[ch];
                next_v[4 * p + ch] = var_out[3 * p + ch] = v;
                next_g[4 * p + ch] = n[ch];
                next_p[4 * p + ch] = P[ch];
                next_m[4 * p + ch] = m2[ch];
            }
            next_c[4 * p + 3] = No;
            next_v[4 * p + 3] = 0.0f;
            std::memcpy(next_g + 4 * p + 3, &id, 4);
            next_p[4 * p + 3] = 0.0f;
            next_m[4 * p + 3] = W2;
            if (len_out) len_out[p] = No;
            if (w2_out) w2_out[p] = W2;
        }
}

} // extern "C"
