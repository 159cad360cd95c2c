// A plain C++ restatement of temporal accumulation with a resampling mode, DESIGN.md §4.26 over §4.15 (the plain step) and §4.16
// (the moments step), written from those sections; it includes no library header.  Built by tests/temporal_cubic_ref.py with
// `g++ -O2 -ffp-contract=off` as a shared object, as tests/temporal_mirror.cpp is.  In mode 0 it must equal tests/temporal_mirror.cpp
// and tests/temporal_moments_mirror.cpp bit for bit (tests/test_temporal_cubic_cpu.py holds it to them); in mode 1 it is held to the
// hand-derived answers of tests/temporal_cubic_cases.py and to the f64 statement of tests/temporal_cubic_f64.py, and the GPU tests
// hold the device to it bit for bit.  The host part of a step (the camera's matrix) is §4.15's and comes from
// tests/temporal_mirror.cpp through tests/temporal_ref.py.
//
// §4.26 in short.  §4.15 steps 1-3 run as they are: B, H, Hv (moments: Q, HW), HN over the accepted ones of the four taps.  The
// cubic path is TAKEN where the step is not static, B >= 2^-6, all sixteen taps (x0 + i, y0 + j), i, j in -1 .. 2, lie inside the
// frame and each passes step 3's acceptance.  Weights of f: w-1 = f·fma(f, fma(-0.5, f, 1), -0.5), w0 = fma(f², fma(1.5, f, -2.5), 1),
// w1 = f·fma(f, fma(-1.5, f, 2), 0.5), w2 = f²·fma(0.5, f, -0.5).  j outer, i inner from +0: b = wx_i·wy_j, W = W + b,
// C = fma(b, c_q, C); hc = C / W; lo, hi over the four inner taps in tap order (lo = c < lo ? c : lo, hi = c > hi ? c : hi);
// h = hc < lo ? lo : (hc > hi ? hi : hc).  Moments: m2 likewise.  Everything else — the variance or W2, the length — is bilinear.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace {

inline float dot3(const float* a, const float* b) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }
const float VCAP = 4294967296.0f;
const float BMIN = 0.015625f; // 2^-6
inline float clampv(float t) { return !(t < VCAP) ? VCAP : (t > 0.0f ? t : 0.0f); }

inline void weights(float f, float* w) {
    const float f2 = f * f;
    w[0] = f * std::fmaf(f, std::fmaf(-0.5f, f, 1.0f), -0.5f);
    w[1] = std::fmaf(f2, std::fmaf(1.5f, f, -2.5f), 1.0f);
    w[2] = f * std::fmaf(f, std::fmaf(-1.5f, f, 2.0f), 0.5f);
    w[3] = f2 * std::fmaf(0.5f, f, -0.5f);
}

// What a pixel with id >= 0 of a handle with history finds: found (B >= 2^-6), the history's colour h, the second record's three
// channels x (the plain step's variance, the moments step's m2) and its fourth xw (the moments step's W2), the length hN, and whether
// h (and, with cubic_x, x) came from the sixteen taps.
struct Hist {
    bool found;
    float h[3], x[3], xw, hN;
    uint8_t taken;
};

struct Frame {
    const float *prev_c, *prev_x, *prev_g, *prev_p; // records of 4 floats per pixel
    uint32_t width, height;
    const float *M, *from;
    float cm, r2;
};

Hist gather(const Frame& fr, long px, long py, int32_t id, const float* n, const float* P, bool is_static, int mode, bool cubic_x) {
    Hist out{};
    const long W_ = (long)fr.width, H_ = (long)fr.height;
    float w[3];
    for (int j = 0; j < 3; ++j) w[j] = P[j] - fr.from[j];
    const float lim = fr.r2 * dot3(w, w);
    auto accepts = [&](long qx, long qy) {
        if (qx < 0 || qx >= W_ || qy < 0 || qy >= H_) return false;
        const size_t q = (size_t)qy * fr.width + qx;
        int32_t qid;
        std::memcpy(&qid, fr.prev_g + 4 * q + 3, 4);
        if (qid != id) return false;
        if (!(dot3(fr.prev_g + 4 * q, n) >= fr.cm)) return false;
        const float d[3] = {fr.prev_p[4 * q] - P[0], fr.prev_p[4 * q + 1] - P[1], fr.prev_p[4 * q + 2] - P[2]};
        return dot3(d, d) <= lim;
    };
    float B = 0.0f, H[3] = {0.0f, 0.0f, 0.0f}, X[3] = {0.0f, 0.0f, 0.0f}, XW = 0.0f, HN = 0.0f;
    auto tap = [&](long qx, long qy, float b) {
        if (!accepts(qx, qy)) return;
        const size_t q = (size_t)qy * fr.width + qx;
        B = B + b;
        for (int ch = 0; ch < 3; ++ch) {
            H[ch] = std::fmaf(b, fr.prev_c[4 * q + ch], H[ch]);
            X[ch] = std::fmaf(b, fr.prev_x[4 * q + ch], X[ch]);
        }
        HN = std::fmaf(b, fr.prev_c[4 * q + 3], HN);
        XW = std::fmaf(b, fr.prev_x[4 * q + 3], XW);
    };
    bool moved = false;
    long x0 = 0, y0 = 0;
    float fx = 0.0f, fy = 0.0f;
    if (is_static) {
        tap(px, py, 1.0f);
    } else {
        const float al = std::fmaf(fr.M[2], w[2], std::fmaf(fr.M[1], w[1], fr.M[0] * w[0]));
        const float be = std::fmaf(fr.M[5], w[2], std::fmaf(fr.M[4], w[1], fr.M[3] * w[0]));
        const float ga = std::fmaf(fr.M[8], w[2], std::fmaf(fr.M[7], w[1], fr.M[6] * w[0]));
        if (ga > 0.0f) {
            const float x = al / ga, y = be / ga;
            if (x > -1.0f && x < (float)fr.width && y > -1.0f && y < (float)fr.height) {
                const float fx0 = std::floor(x), fy0 = std::floor(y);
                fx = x - fx0, fy = y - fy0;
                x0 = (long)fx0, y0 = (long)fy0;
                moved = true;
                for (int j = 0; j < 2; ++j)
                    for (int i = 0; i < 2; ++i) tap(x0 + i, y0 + j, (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy));
            }
        }
    }
    if (!(B >= BMIN)) return out;
    out.found = true;
    for (int ch = 0; ch < 3; ++ch) out.h[ch] = H[ch] / B, out.x[ch] = X[ch] / B;
    out.xw = XW / B, out.hN = HN / B;
    if (mode != 1 || !moved) return out;
    // §4.26: taken where all sixteen taps are inside the frame and accepted
    for (long j = -1; j <= 2; ++j)
        for (long i = -1; i <= 2; ++i)
            if (!accepts(x0 + i, y0 + j)) return out;
    float wx[4], wy[4];
    weights(fx, wx);
    weights(fy, wy);
    float Wt = 0.0f, C[3] = {0.0f, 0.0f, 0.0f}, D[3] = {0.0f, 0.0f, 0.0f};
    for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 4; ++i) {
            const size_t q = (size_t)(y0 + j - 1) * fr.width + (size_t)(x0 + i - 1);
            const float b = wx[i] * wy[j];
            Wt = Wt + b;
            for (int ch = 0; ch < 3; ++ch) {
                C[ch] = std::fmaf(b, fr.prev_c[4 * q + ch], C[ch]);
                D[ch] = std::fmaf(b, fr.prev_x[4 * q + ch], D[ch]);
            }
        }
    auto resolve = [&](const float* rec, const float* S, float* dst) {
        for (int ch = 0; ch < 3; ++ch) {
            const float hc = S[ch] / Wt;
            float lo = 0.0f, hi = 0.0f;
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < 2; ++i) {
                    const float c = rec[4 * ((size_t)(y0 + j) * fr.width + (size_t)(x0 + i)) + ch];
                    if (i == 0 && j == 0) lo = hi = c;
                    lo = c < lo ? c : lo;
                    hi = c > hi ? c : hi;
                }
            dst[ch] = hc < lo ? lo : (hc > hi ? hi : hc);
        }
    };
    resolve(fr.prev_c, C, out.h);
    if (cubic_x) resolve(fr.prev_x, D, out.x);
    out.taken = 1;
    return out;
}

struct Blend {
    float a, k, N;
};
inline Blend blend_head(float hN, float spp, float am, float nm) {
    const float Ns = hN + spp;
    const float a0 = spp / Ns;
    const float a = a0 < am ? am : a0;
    return Blend{a, 1.0f - a, Ns > nm ? nm : Ns};
}

} // namespace

extern "C" {

// The plain step (§4.15 with §4.26's mode).  As tests/temporal_mirror.cpp's temporal_mirror_step, plus mode (0 bilinear, 1 cubic)
// and taken (height·width bytes, or null).
void temporal_cubic_mirror_step(const float* rgb, const float* var, const int32_t* index, const float* normal, const float* point,
                                const float* prev_c, const float* prev_v, const float* prev_g, const float* prev_p, float* next_c,
                                float* next_v, float* next_g, float* next_p, float* rgb_out, float* var_out, float* len_out,
                                uint32_t width, uint32_t height, int has_history, int is_static, const float* M, const float* from,
                                float spp, float am, float nm, float cm, float r2, int mode, uint8_t* taken) {
    const Frame fr{prev_c, prev_v, prev_g, prev_p, width, height, M, from, cm, r2};
    for (long py = 0; py < (long)height; ++py)
        for (long px = 0; px < (long)width; ++px) {
            const size_t p = (size_t)py * width + px;
            const float c[3] = {rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]};
            const float s[3] = {clampv(var[3 * p]), clampv(var[3 * p + 1]), clampv(var[3 * p + 2])};
            const int32_t id = index[p];
            const float* n = normal + 3 * p;
            const float* P = point + 3 * p;
            float co[3] = {c[0], c[1], c[2]}, vo[3] = {s[0], s[1], s[2]}, No = spp;
            uint8_t took = 0;
            if (id >= 0 && has_history) {
                const Hist hi = gather(fr, px, py, id, n, P, is_static != 0, mode, false);
                if (hi.found) {
                    const Blend b = blend_head(hi.hN, spp, am, nm);
                    for (int ch = 0; ch < 3; ++ch) {
                        co[ch] = std::fmaf(b.a, c[ch] - hi.h[ch], hi.h[ch]);
                        vo[ch] = std::fmaf(b.a * b.a, s[ch], (b.k * b.k) * hi.x[ch]);
                    }
                    No = b.N;
                    took = hi.taken;
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
            if (taken) taken[p] = took;
        }
}

// The moments step (§4.16 with §4.26's mode).  As tests/temporal_moments_mirror.cpp's step, plus mode and taken.
void temporal_cubic_mirror_step_moments(const float* rgb, const int32_t* index, const float* normal, const float* point,
                                        const float* prev_c, const float* prev_g, const float* prev_p, const float* prev_m,
                                        float* next_c, float* next_v, float* next_g, float* next_p, float* next_m, float* rgb_out,
                                        float* var_out, float* len_out, float* w2_out, uint32_t width, uint32_t height, int has_history,
                                        int is_static, const float* M, const float* from, float spp, float am, float nm, float cm,
                                        float r2, float wm, float mt, int mode, uint8_t* taken) {
    const Frame fr{prev_c, prev_m, prev_g, prev_p, width, height, M, from, cm, r2};
    for (long py = 0; py < (long)height; ++py)
        for (long px = 0; px < (long)width; ++px) {
            const size_t p = (size_t)py * width + px;
            const float c[3] = {rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]};
            const int32_t id = index[p];
            const float* n = normal + 3 * p;
            const float* P = point + 3 * p;
            float co[3] = {c[0], c[1], c[2]}, m2[3] = {c[0] * c[0], c[1] * c[1], c[2] * c[2]}, No = spp, W2 = 1.0f;
            uint8_t took = 0;
            if (id >= 0 && has_history) {
                const Hist hi = gather(fr, px, py, id, n, P, is_static != 0, mode, true);
                if (hi.found) {
                    const Blend b = blend_head(hi.hN, spp, am, nm);
                    for (int ch = 0; ch < 3; ++ch) {
                        co[ch] = std::fmaf(b.a, c[ch] - hi.h[ch], hi.h[ch]);
                        m2[ch] = std::fmaf(b.a, c[ch] * c[ch] - hi.x[ch], hi.x[ch]);
                    }
                    W2 = std::fmaf(b.k * b.k, hi.xw, b.a * b.a);
                    No = b.N;
                    took = hi.taken;
                }
            }
            float vt[3], vs[3] = {VCAP, VCAP, VCAP};
            for (int ch = 0; ch < 3; ++ch) {
                const float e = m2[ch] - (co[ch] * co[ch]);
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
            if (taken) taken[p] = took;
        }
}

// The four weights of f, for the hand cases.
void temporal_cubic_mirror_weights(float f, float* w) { weights(f, w); }

} // extern "C"
