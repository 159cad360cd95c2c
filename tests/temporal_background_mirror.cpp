// A plain C++ restatement of temporal accumulation's background mode, DESIGN.md §4.27 (on §4.15 for the plain handle, on §4.16
// for the moments handle, and on §4.23 for both with a count per pixel), written from those sections; it includes no library
// header.  Built by tests/temporal_background_ref.py with `g++ -O2 -ffp-contract=off` as a shared object, as
// tests/temporal_mirror.cpp is; it is held, independently of the device, to the hand-derived answers of
// tests/temporal_background_cases.py, in INPUT mode to the mirrors of the four existing steps bit for bit, and to the f64 statement
// of tests/temporal_background_f64.py; the GPU tests hold the device to it bit for bit.  §4.15's host part (M and from) comes from
// tests/temporal_mirror.cpp through tests/temporal_ref.py; §4.27's host part (G) is restated here.
//
// §4.27 in short.  mode 0 (INPUT): a pixel with id < 0 has no history.  mode 1 (ACCUMULATE): it projects its own centre (x, y, 1)
// through G — three rows of two FMAs —, takes §4.15's four taps there and accepts those inside the frame whose history index is
// < 0 (with counts: and whose length is > 0); a static step takes the pixel's own record with b = 1.  From the sums on it is the
// hit pixel's step.  Moments: v_out = vt where it found history and !(W2 > wm), else +0; never the spatial estimate.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace {

inline float dot3(const float* a, const float* b) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }
const float VCAP = 4294967296.0f;
const float BMIN = 0.015625f; // 2^-6
inline float clampv(float t) { return !(t < VCAP) ? VCAP : (t > 0.0f ? t : 0.0f); }

struct Sums {
    float B = 0.0f, S[2][4] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};
};

struct Frame {
    uint32_t width, height;
    int has_history, is_static, mode, live; // live: a counts step (a record of length 0 holds no samples)
    const float *M, *from, *G;
    float am, nm, cm, r2;
    const float *prev_g, *prev_p, *rec0, *rec1; // rec0 = {c, N}; rec1 = {v, 0} (plain) or {m2, W2} (moments)
};

// §4.15 step 3 from the position (x, y) on: the four taps in the order j outer, i inner; accept(q) is the tap's own test.
template <class Accept> void taps(const Frame& f, float x, float y, Sums& acc, const Accept& accept) {
    const float x0 = std::floor(x), y0 = std::floor(y);
    const float fx = x - x0, fy = y - y0;
    for (int j = 0; j < 2; ++j)
        for (int i = 0; i < 2; ++i) {
            const long qx = (long)x0 + i, qy = (long)y0 + j;
            const float b = (i ? fx : 1.0f - fx) * (j ? fy : 1.0f - fy);
            if (qx < 0 || qx >= (long)f.width || qy < 0 || qy >= (long)f.height) continue;
            const size_t q = (size_t)qy * f.width + qx;
            if (!accept(q)) continue;
            acc.B = acc.B + b;
            for (int k = 0; k < 4; ++k) {
                acc.S[0][k] = std::fmaf(b, f.rec0[4 * q + k], acc.S[0][k]);
                acc.S[1][k] = std::fmaf(b, f.rec1[4 * q + k], acc.S[1][k]);
            }
        }
}

inline void own(const Frame& f, size_t q, Sums& acc) { // the static step's one tap, b = 1
    acc.B = acc.B + 1.0f;
    for (int k = 0; k < 4; ++k) {
        acc.S[0][k] = std::fmaf(1.0f, f.rec0[4 * q + k], acc.S[0][k]);
        acc.S[1][k] = std::fmaf(1.0f, f.rec1[4 * q + k], acc.S[1][k]);
    }
}

inline bool in_range(const Frame& f, float x, float y) { return x > -1.0f && x < (float)f.width && y > -1.0f && y < (float)f.height; }

inline int32_t prev_id(const Frame& f, size_t q) {
    int32_t id;
    std::memcpy(&id, f.prev_g + 4 * q + 3, 4);
    return id;
}

// §4.15 steps 2 and 3 (with §4.23's rule 1 where live) for a pixel with id >= 0.
Sums gather_hit(const Frame& f, long px, long py, int32_t id, const float* n, const float* P) {
    Sums acc;
    float w[3];
    for (int j = 0; j < 3; ++j) w[j] = P[j] - f.from[j];
    const float lim = f.r2 * dot3(w, w);
    auto accept = [&](size_t q) {
        if (prev_id(f, q) != id) return false;
        if (!(dot3(f.prev_g + 4 * q, n) >= f.cm)) return false;
        const float d[3] = {f.prev_p[4 * q] - P[0], f.prev_p[4 * q + 1] - P[1], f.prev_p[4 * q + 2] - P[2]};
        if (!(dot3(d, d) <= lim)) return false;
        return !f.live || f.rec0[4 * q + 3] > 0.0f;
    };
    if (f.is_static) {
        const size_t p = (size_t)py * f.width + px;
        if (accept(p)) own(f, p, acc);
        return acc;
    }
    const float* M = f.M;
    const float al = std::fmaf(M[2], w[2], std::fmaf(M[1], w[1], M[0] * w[0]));
    const float be = std::fmaf(M[5], w[2], std::fmaf(M[4], w[1], M[3] * w[0]));
    const float ga = std::fmaf(M[8], w[2], std::fmaf(M[7], w[1], M[6] * w[0]));
    if (!(ga > 0.0f)) return acc;
    const float x = al / ga, y = be / ga;
    if (!in_range(f, x, y)) return acc;
    taps(f, x, y, acc, accept);
    return acc;
}

// §4.27 rules 1 and 2 for a pixel with id < 0 in ACCUMULATE mode.
Sums gather_background(const Frame& f, long px, long py) {
    Sums acc;
    auto accept = [&](size_t q) { return prev_id(f, q) < 0 && (!f.live || f.rec0[4 * q + 3] > 0.0f); };
    if (f.is_static) {
        const size_t p = (size_t)py * f.width + px;
        if (accept(p)) own(f, p, acc);
        return acc;
    }
    const float* G = f.G;
    const float xf = (float)px, yf = (float)py;
    const float al = std::fmaf(G[1], yf, std::fmaf(G[0], xf, G[2]));
    const float be = std::fmaf(G[4], yf, std::fmaf(G[3], xf, G[5]));
    const float ga = std::fmaf(G[7], yf, std::fmaf(G[6], xf, G[8]));
    if (!(ga > 0.0f)) return acc;
    const float x = al / ga, y = be / ga;
    if (!in_range(f, x, y)) return acc;
    taps(f, x, y, acc, accept);
    return acc;
}

Sums gather(const Frame& f, long px, long py, int32_t id, const float* n, const float* P) {
    if (!f.has_history) return Sums();
    if (id >= 0) return gather_hit(f, px, py, id, n, P);
    return f.mode == 1 ? gather_background(f, px, py) : Sums();
}

} // namespace

extern "C" {

// §4.27's host part: prev and cam are the twelve doubles look_from, px_du, px_dv, px_origin of the previous and of this step's camera.
void temporal_background_mirror_G(const double* prev, const double* cam, float* G) {
    const double *u = prev + 3, *v = prev + 6;
    const double a[3] = {prev[9] - prev[0], prev[10] - prev[1], prev[11] - prev[2]};
    auto cross = [](const double* p, const double* q, double* o) {
        o[0] = p[1] * q[2] - p[2] * q[1];
        o[1] = p[2] * q[0] - p[0] * q[2];
        o[2] = p[0] * q[1] - p[1] * q[0];
    };
    double r[3][3];
    cross(v, a, r[0]);
    cross(a, u, r[1]);
    cross(u, v, r[2]);
    const double det = (u[0] * r[0][0] + u[1] * r[0][1]) + u[2] * r[0][2];
    const double c2[3] = {cam[9] - cam[0], cam[10] - cam[1], cam[11] - cam[2]};
    const double* c[3] = {cam + 3, cam + 6, c2};
    for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 3; ++j) G[3 * k + j] = (float)(((r[k][0] * c[j][0] + r[k][1] * c[j][1]) + r[k][2] * c[j][2]) / det);
}

// One step of a plain handle.  counts: NULL for the step with one spp, else height·width uint32 (then spp is not read).
void temporal_background_mirror_step(const float* rgb, const float* var, const uint32_t* counts, const int32_t* index,
                                     const float* normal, const float* point, const float* prev_c, const float* prev_v,
                                     const float* prev_g, const float* prev_p, float* next_c, float* next_v, float* next_g,
                                     float* next_p, float* rgb_out, float* var_out, float* len_out, uint32_t width, uint32_t height,
                                     int has_history, int is_static, int mode, const float* M, const float* from, const float* G,
                                     float spp, float am, float nm, float cm, float r2) {
    const Frame f{width, height, has_history, is_static, mode, counts != nullptr, M, from, G, am, nm, cm, r2, prev_g, prev_p, prev_c, prev_v};
    for (long py = 0; py < (long)height; ++py)
        for (long px = 0; px < (long)width; ++px) {
            const size_t p = (size_t)py * width + px;
            const float* c = rgb + 3 * p;
            const float s[3] = {clampv(var[3 * p]), clampv(var[3 * p + 1]), clampv(var[3 * p + 2])};
            const int32_t id = index[p];
            const float *n = normal + 3 * p, *P = point + 3 * p;
            const float cnt = counts ? (float)counts[p] : spp;
            float co[3] = {c[0], c[1], c[2]}, vo[3] = {s[0], s[1], s[2]}, No = cnt;
            const Sums acc = gather(f, px, py, id, n, P);
            if (acc.B >= BMIN) {
                const float hN = acc.S[0][3] / acc.B;
                const float Ns = hN + cnt;
                if (!counts || cnt > 0.0f) {
                    const float a0 = cnt / Ns;
                    const float a = a0 < am ? am : a0;
                    const float k = 1.0f - a;
                    for (int ch = 0; ch < 3; ++ch) {
                        const float h = acc.S[0][ch] / acc.B, hv = acc.S[1][ch] / acc.B;
                        co[ch] = std::fmaf(a, c[ch] - h, h);
                        vo[ch] = std::fmaf(a * a, s[ch], (k * k) * hv);
                    }
                } else {
                    for (int ch = 0; ch < 3; ++ch) co[ch] = acc.S[0][ch] / acc.B, vo[ch] = acc.S[1][ch] / acc.B;
                }
                No = Ns > nm ? nm : Ns;
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

// One step of a moments handle.  counts: as above.
void temporal_background_mirror_step_moments(const float* rgb, const uint32_t* counts, const int32_t* index, const float* normal,
                                             const float* point, const float* prev_c, const float* prev_g, const float* prev_p,
                                             const float* prev_m, float* next_c, float* next_v, float* next_g, float* next_p,
                                             float* next_m, float* rgb_out, float* var_out, float* len_out, float* w2_out,
                                             uint32_t width, uint32_t height, int has_history, int is_static, int mode, const float* M,
                                             const float* from, const float* G, float spp, float am, float nm, float cm, float r2,
                                             float wm, float mt) {
    const Frame f{width, height, has_history, is_static, mode, counts != nullptr, M, from, G, am, nm, cm, r2, prev_g, prev_p, prev_c, prev_m};
    for (long py = 0; py < (long)height; ++py)
        for (long px = 0; px < (long)width; ++px) {
            const size_t p = (size_t)py * width + px;
            const float* c = rgb + 3 * p;
            const int32_t id = index[p];
            const float *n = normal + 3 * p, *P = point + 3 * p;
            const float cnt = counts ? (float)counts[p] : spp;
            float co[3] = {c[0], c[1], c[2]}, m2[3] = {c[0] * c[0], c[1] * c[1], c[2] * c[2]}, No = cnt, W2 = 1.0f;
            const Sums acc = gather(f, px, py, id, n, P);
            const bool found = acc.B >= BMIN;
            if (found) {
                const float hN = acc.S[0][3] / acc.B, hW = acc.S[1][3] / acc.B;
                const float Ns = hN + cnt;
                if (!counts || cnt > 0.0f) {
                    const float a0 = cnt / Ns;
                    const float a = a0 < am ? am : a0;
                    const float k = 1.0f - a;
                    for (int ch = 0; ch < 3; ++ch) {
                        const float h = acc.S[0][ch] / acc.B, hq = acc.S[1][ch] / acc.B;
                        co[ch] = std::fmaf(a, c[ch] - h, h);
                        m2[ch] = std::fmaf(a, c[ch] * c[ch] - hq, hq);
                    }
                    W2 = std::fmaf(k * k, hW, a * a);
                } else {
                    for (int ch = 0; ch < 3; ++ch) co[ch] = acc.S[0][ch] / acc.B, m2[ch] = acc.S[1][ch] / acc.B;
                    W2 = hW;
                }
                No = Ns > nm ? nm : Ns;
            }
            // §4.16 step 3
            float vt[3], vs[3] = {VCAP, VCAP, VCAP};
            for (int ch = 0; ch < 3; ++ch) {
                const float e = m2[ch] - (co[ch] * co[ch]);
                const float ep = e > 0.0f ? e : 0.0f;
                vt[ch] = clampv((ep * W2) / (1.0f - W2));
            }
            // §4.16 step 4, where id >= 0 only (with counts: over the positions that were sampled)
            const bool spatial = id >= 0 && W2 > wm;
            if (spatial) {
                float S0 = 0.0f, S1[3] = {0.0f, 0.0f, 0.0f}, S2[3] = {0.0f, 0.0f, 0.0f};
                for (long j = -3; j <= 3; ++j)
                    for (long i = -3; i <= 3; ++i) {
                        const long qx = px + i, qy = py + j;
                        if (qx < 0 || qx >= (long)width || qy < 0 || qy >= (long)height) continue;
                        const size_t q = (size_t)qy * width + qx;
                        if (index[q] != id) continue;
                        if (counts && !(counts[q] > 0)) continue;
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
            // step 5: a hit pixel's selection; the background's is §4.27 rule 3's
            const bool bg_vt = id < 0 && mode == 1 && found && !(W2 > wm);
            for (int ch = 0; ch < 3; ++ch) {
                const float v = id < 0 ? (bg_vt ? vt[ch] : 0.0f) : (spatial ? vs[ch] : vt[ch]);
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
