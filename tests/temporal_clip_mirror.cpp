// A plain C++ restatement of temporal accumulation's clip mode, DESIGN.md §4.28 (on §4.15 for the plain handle, on §4.16 for the
// moments handle, and on §4.27 for both in background-accumulate mode), written from those sections; it includes no library
// header.  Built by tests/temporal_clip_ref.py with `g++ -O2 -ffp-contract=off` as a shared object, as
// tests/temporal_background_mirror.cpp is; it is held, independently of the device, to the hand-derived answers of
// tests/temporal_clip_cases.py and, with gamma = +inf, to the mirrors of the plain, the moments and the background steps bit for
// bit; the GPU tests hold the device to it bit for bit.  The host parts (§4.15's M and from, §4.27's G) come from
// tests/temporal_mirror.cpp and tests/temporal_background_mirror.cpp through their Python sides.
//
// §4.28 in short.  clip 0 (OFF): the step of §4.15 / §4.16 / §4.27.  clip 1 (VARIANCE): in a MOVING step, a pixel that found
// history (B >= 2^-6) — a hit pixel, or with background 1 a pixel with id < 0 — sums the current frame over its 7x7 neighbourhood
// (j outer, ascending; a hit pixel: the taps inside the frame with its index, and the centre or dot(n(q), n) >= cm; a background
// pixel: the taps inside the frame with index < 0), and where S0 >= min_taps clamps each channel of the history mean h = H/B to
// mu ± g·sqrt(vn) before the blend.  Moments: a clipped channel's hq becomes fma(hk, hk, max(hq − h·h, 0)).
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
    int has_history, is_static, background, clip;
    const float *M, *from, *G;
    float am, nm, cm, r2, g, cmt; // g, cmt: f32 of the clip's gamma and min_taps
    const float *prev_g, *prev_p, *rec0, *rec1; // rec0 = {c, N}; rec1 = {v, 0} (plain) or {m2, W2} (moments)
    const float* rgb;                           // the current frame and its guides
    const int32_t* index;
    const float* normal;
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

// §4.15 steps 2 and 3 for a pixel with id >= 0.
Sums gather_hit(const Frame& f, long px, long py, int32_t id, const float* n, const float* P) {
    Sums acc;
    float w[3];
    for (int j = 0; j < 3; ++j) w[j] = P[j] - f.from[j];
    const float lim = f.r2 * dot3(w, w);
    auto accept = [&](size_t q) {
        if (prev_id(f, q) != id) return false;
        if (!(dot3(f.prev_g + 4 * q, n) >= f.cm)) return false;
        const float d[3] = {f.prev_p[4 * q] - P[0], f.prev_p[4 * q + 1] - P[1], f.prev_p[4 * q + 2] - P[2]};
        return dot3(d, d) <= lim;
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
    auto accept = [&](size_t q) { return prev_id(f, q) < 0; };
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
    return f.background == 1 ? gather_background(f, px, py) : Sums();
}

// §4.16 step 4's sums and §4.28 rule 1's: the current frame over the 7x7 neighbourhood of (px, py).
struct Hood {
    float S0 = 0.0f, S1[3] = {0.0f, 0.0f, 0.0f}, S2[3] = {0.0f, 0.0f, 0.0f};
};

Hood neighbourhood(const Frame& f, long px, long py, int32_t id, const float* n) {
    Hood h;
    const size_t p = (size_t)py * f.width + px;
    for (long j = -3; j <= 3; ++j)
        for (long i = -3; i <= 3; ++i) {
            const long qx = px + i, qy = py + j;
            if (qx < 0 || qx >= (long)f.width || qy < 0 || qy >= (long)f.height) continue;
            const size_t q = (size_t)qy * f.width + qx;
            if (id < 0) {
                if (!(f.index[q] < 0)) continue; // a background pixel: the misses, with no normal test
            } else {
                if (f.index[q] != id) continue;
                if (!(q == p || dot3(f.normal + 3 * q, n) >= f.cm)) continue;
            }
            h.S0 = h.S0 + 1.0f;
            for (int ch = 0; ch < 3; ++ch) {
                h.S1[ch] = h.S1[ch] + f.rgb[3 * q + ch];
                h.S2[ch] = std::fmaf(f.rgb[3 * q + ch], f.rgb[3 * q + ch], h.S2[ch]);
            }
        }
    return h;
}

// §4.28 rule 2 for one channel: hk, and whether h lay outside the box.
inline float clip_channel(const Frame& f, const Hood& nb, int ch, float h, bool& clipped) {
    clipped = false;
    if (!(nb.S0 >= f.cmt)) return h;
    const float mu = nb.S1[ch] / nb.S0;
    const float d = nb.S2[ch] / nb.S0 - mu * mu;
    const float dp = d > 0.0f ? d : 0.0f;
    const float vn = (dp * nb.S0) / (nb.S0 - 1.0f);
    const float sd = std::sqrt(vn);
    const float e = f.g * sd;
    const float lo = mu - e, hi = mu + e;
    clipped = h < lo || h > hi;
    return h < lo ? lo : (h > hi ? hi : h);
}

// Does the rule apply to this step at all?  (Then to every pixel that found history.)
inline bool clips(const Frame& f) { return f.clip == 1 && f.has_history && !f.is_static; }

} // namespace

extern "C" {

// One step of a plain handle.  clipped_out: height·width bytes, or NULL.
void temporal_clip_mirror_step(const float* rgb, const float* var, const int32_t* index, const float* normal, const float* point,
                               const float* prev_c, const float* prev_v, const float* prev_g, const float* prev_p, float* next_c,
                               float* next_v, float* next_g, float* next_p, float* rgb_out, float* var_out, float* len_out,
                               uint8_t* clipped_out, uint32_t width, uint32_t height, int has_history, int is_static, int background,
                               int clip, const float* M, const float* from, const float* G, float spp, float am, float nm, float cm,
                               float r2, float gamma, float clip_min_taps) {
    const Frame f{width, height, has_history, is_static, background, clip, M, from, G, am, nm, cm, r2, gamma, clip_min_taps,
                  prev_g, prev_p, prev_c, prev_v, rgb, index, normal};
    for (long py = 0; py < (long)height; ++py)
        for (long px = 0; px < (long)width; ++px) {
            const size_t p = (size_t)py * width + px;
            const float* c = rgb + 3 * p;
            const float s[3] = {clampv(var[3 * p]), clampv(var[3 * p + 1]), clampv(var[3 * p + 2])};
            const int32_t id = index[p];
            const float *n = normal + 3 * p, *P = point + 3 * p;
            float co[3] = {c[0], c[1], c[2]}, vo[3] = {s[0], s[1], s[2]}, No = spp;
            bool any = false;
            const Sums acc = gather(f, px, py, id, n, P);
            if (acc.B >= BMIN) {
                const float hN = acc.S[0][3] / acc.B;
                const float Ns = hN + spp;
                const float a0 = spp / Ns;
                const float a = a0 < am ? am : a0;
                const float k = 1.0f - a;
                Hood nb;
                if (clips(f)) nb = neighbourhood(f, px, py, id, n);
                for (int ch = 0; ch < 3; ++ch) {
                    const float h = acc.S[0][ch] / acc.B, hv = acc.S[1][ch] / acc.B;
                    bool cl = false;
                    const float hk = clips(f) ? clip_channel(f, nb, ch, h, cl) : h;
                    any = any || cl;
                    co[ch] = std::fmaf(a, c[ch] - hk, hk);
                    vo[ch] = std::fmaf(a * a, s[ch], (k * k) * hv);
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
            if (clipped_out) clipped_out[p] = any ? 1 : 0;
        }
}

// One step of a moments handle.
void temporal_clip_mirror_step_moments(const float* rgb, const int32_t* index, const float* normal, const float* point,
                                       const float* prev_c, const float* prev_g, const float* prev_p, const float* prev_m, float* next_c,
                                       float* next_v, float* next_g, float* next_p, float* next_m, float* rgb_out, float* var_out,
                                       float* len_out, float* w2_out, uint8_t* clipped_out, uint32_t width, uint32_t height,
                                       int has_history, int is_static, int background, int clip, const float* M, const float* from,
                                       const float* G, float spp, float am, float nm, float cm, float r2, float wm, float mt, float gamma,
                                       float clip_min_taps) {
    const Frame f{width, height, has_history, is_static, background, clip, M, from, G, am, nm, cm, r2, gamma, clip_min_taps,
                  prev_g, prev_p, prev_c, prev_m, rgb, index, normal};
    for (long py = 0; py < (long)height; ++py)
        for (long px = 0; px < (long)width; ++px) {
            const size_t p = (size_t)py * width + px;
            const float* c = rgb + 3 * p;
            const int32_t id = index[p];
            const float *n = normal + 3 * p, *P = point + 3 * p;
            float co[3] = {c[0], c[1], c[2]}, m2[3] = {c[0] * c[0], c[1] * c[1], c[2] * c[2]}, No = spp, W2 = 1.0f;
            bool any = false;
            const Sums acc = gather(f, px, py, id, n, P);
            const bool found = acc.B >= BMIN;
            if (found) {
                const float hN = acc.S[0][3] / acc.B, hW = acc.S[1][3] / acc.B;
                const float Ns = hN + spp;
                const float a0 = spp / Ns;
                const float a = a0 < am ? am : a0;
                const float k = 1.0f - a;
                Hood nb;
                if (clips(f)) nb = neighbourhood(f, px, py, id, n);
                for (int ch = 0; ch < 3; ++ch) {
                    const float h = acc.S[0][ch] / acc.B;
                    float hq = acc.S[1][ch] / acc.B;
                    bool cl = false;
                    const float hk = clips(f) ? clip_channel(f, nb, ch, h, cl) : h;
                    if (cl) { // rule 4: the history keeps its spread about the new mean
                        const float t = hq - h * h;
                        const float tp = t > 0.0f ? t : 0.0f;
                        hq = std::fmaf(hk, hk, tp);
                    }
                    any = any || cl;
                    co[ch] = std::fmaf(a, c[ch] - hk, hk);
                    m2[ch] = std::fmaf(a, c[ch] * c[ch] - hq, hq);
                }
                W2 = std::fmaf(k * k, hW, a * a);
                No = Ns > nm ? nm : Ns;
            }
            // §4.16 step 3
            float vt[3], vs[3] = {VCAP, VCAP, VCAP};
            for (int ch = 0; ch < 3; ++ch) {
                const float e = m2[ch] - (co[ch] * co[ch]);
                const float ep = e > 0.0f ? e : 0.0f;
                vt[ch] = clampv((ep * W2) / (1.0f - W2));
            }
            // §4.16 step 4, where id >= 0 only: the same sums as the clip's
            const bool spatial = id >= 0 && W2 > wm;
            if (spatial) {
                const Hood nb = neighbourhood(f, px, py, id, n);
                if (nb.S0 >= mt)
                    for (int ch = 0; ch < 3; ++ch) {
                        const float mu = nb.S1[ch] / nb.S0;
                        const float d = nb.S2[ch] / nb.S0 - mu * mu;
                        const float dp = d > 0.0f ? d : 0.0f;
                        vs[ch] = clampv(((dp * nb.S0) / (nb.S0 - 1.0f)) * W2);
                    }
            }
            // step 5: a hit pixel's selection; the background's is §4.27 rule 3's
            const bool bg_vt = id < 0 && background == 1 && found && !(W2 > wm);
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
            if (clipped_out) clipped_out[p] = any ? 1 : 0;
        }
}

} // extern "C"
