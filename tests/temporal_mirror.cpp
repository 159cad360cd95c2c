// A plain C++ restatement of temporal accumulation, DESIGN.md §4.15, written from that section; it includes no library header.
// Built by tests/temporal_ref.py with `g++ -O2 -ffp-contract=off` as a shared object, as tests/denoise_guided_mirror.cpp is; it is
// held, independently of the device, to the hand-derived answers of tests/temporal_cases.py, and the GPU tests hold the device to
// it bit for bit.
//
// §4.15 in short.  A history buffer is four arrays of 4 floats per pixel: hc = {c, N}, hv = {v, 0}, hg = {n, bits(index)},
// hp = {P, 0}.  Host, f64: a = px_origin − look_from, rows r0 = v×a, r1 = a×u, r2 = u×v, det = (u_x·r0_x + u_y·r0_y) + u_z·r0_z,
// M[k][j] = f32(rk_j / det), from = f32(look_from).  Device, per pixel: s = clamp(var) as §4.13; no history (output = input,
// N = spp) for background, a handle without history, a failed projection or B not >= 2^-6; taps at (x0 + i, y0 + j) with bilinear
// b, accepted inside the frame with the same index, dot(n_q, n) >= cm and |P_q − P|² <= r2·|P − from|²; B, H, Hv, HN summed by fma in
// tap order and divided by B; Ns = hN + spp, al = max(spp / Ns, am), c = fma(al, c − h, h), v = fma(al·al, s, (k·k)·hv), k = 1 − al,
// N = min(Ns, nm).  A static step has the one tap q = p with b = 1.
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace {

inline float dot3(const float* a, const float* b) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }
inline void cross(const double* p, const double* q, double* o) {
    o[0] = p[1] * q[2] - p[2] * q[1];
    o[1] = p[2] * q[0] - p[0] * q[2];
    o[2] = p[0] * q[1] - p[1] * q[0];
}
const float VCAP = 4294967296.0f;
const float BMIN = 0.015625f; // 2^-6

struct Acc {
    float B, H[3], Hv[3], HN;
};

// Step 2's position: w = P − from, then (x, y, γ) through M.  x and y mean something only where γ > 0.  The step and
// temporal_mirror_project both go through these two, so what the latter reports is what the former uses.
struct Proj {
    float x, y, ga;
};
inline void offset(const float* P, const float* from, float* w) {
    for (int j = 0; j < 3; ++j) w[j] = P[j] - from[j];
}
inline Proj project(const float* M, const float* w) {
    const float al = std::fmaf(M[2], w[2], std::fmaf(M[1], w[1], M[0] * w[0]));
    const float be = std::fmaf(M[5], w[2], std::fmaf(M[4], w[1], M[3] * w[0]));
    const float ga = std::fmaf(M[8], w[2], std::fmaf(M[7], w[1], M[6] * w[0]));
    return Proj{al / ga, be / ga, ga};
}

} // namespace

extern "C" {

// cam: look_from(3), px_du(3), px_dv(3), px_origin(3).  Returns 0 where det is zero or not finite (RAYZ_ERR_BAD_ARG), else 1.
int temporal_mirror_camera(const double* cam, float* M, float* from) {
    const double *lf = cam, *u = cam + 3, *v = cam + 6, *po = cam + 9;
    const double a[3] = {po[0] - lf[0], po[1] - lf[1], po[2] - lf[2]};
    double r[3][3];
    cross(v, a, r[0]);
    cross(a, u, r[1]);
    cross(u, v, r[2]);
    const double det = (u[0] * r[0][0] + u[1] * r[0][1]) + u[2] * r[0][2];
    if (!(det != 0.0) || !std::isfinite(det)) return 0;
    for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 3; ++j) M[3 * k + j] = (float)(r[k][j] / det);
    for (int j = 0; j < 3; ++j) from[j] = (float)lf[j];
    return 1;
}

// The f32 (x, y, γ) that a step projecting with M / from computes for each of `count` points: out[3·i] = x, [3·i + 1] = y, [3·i + 2] = γ
// (x and y as divided, whatever γ is).  For the test of §4.15's accuracy statement.
void temporal_mirror_project(const float* point, size_t count, const float* M, const float* from, float* out) {
    for (size_t i = 0; i < count; ++i) {
        float w[3];
        offset(point + 3 * i, from, w);
        const Proj pr = project(M, w);
        out[3 * i] = pr.x;
        out[3 * i + 1] = pr.y;
        out[3 * i + 2] = pr.ga;
    }
}

// One step.  prev_* : the history the previous step wrote (ignored when !has_history); next_* : the history this step writes.
// mode: 0 = project with M / from (the PREVIOUS camera's), 1 = static.  len_out may be null.
void temporal_mirror_step(const float* rgb, const float* var, const int32_t* index, const float* normal, const float* point,
                          const float* prev_c, const float* prev_v, const float* prev_g, const float* prev_p, float* next_c,
                          float* next_v, float* next_g, float* next_p, float* rgb_out, float* var_out, float* len_out, uint32_t width,
                          uint32_t height, int has_history, int is_static, const float* M, const float* from, float spp, float am,
                          float nm, float cm, float r2) {
    const float Wf = (float)width, Hf = (float)height;
    for (long py = 0; py < (long)height; ++py)
        for (long px = 0; px < (long)width; ++px) {
            const size_t p = (size_t)py * width + px;
            const float c[3] = {rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]};
            float s[3];
            for (int ch = 0; ch < 3; ++ch) {
                const float t = var[3 * p + ch];
                s[ch] = !(t < VCAP) ? VCAP : (t > 0.0f ? t : 0.0f);
            }
            const int32_t id = index[p];
            const float* n = normal + 3 * p;
            const float* P = point + 3 * p;
            float co[3] = {c[0], c[1], c[2]}, vo[3] = {s[0], s[1], s[2]}, No = spp;
            if (id >= 0 && has_history) {
                float w[3];
                offset(P, from, w);
                const float lim = r2 * dot3(w, w);
                Acc acc{0.0f, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}, 0.0f};
                auto tap = [&](long qx, long qy, float b) {
                    if (qx < 0 || qx >= (long)width || qy < 0 || qy >= (long)height) return;
                    const size_t q = (size_t)qy * width + qx;
                    int32_t qid;
                    std::memcpy(&qid, prev_g + 4 * q + 3, 4);
                    if (qid != id) return;
                    if (!(dot3(prev_g + 4 * q, n) >= cm)) return;
                    const float d[3] = {prev_p[4 * q] - P[0], prev_p[4 * q + 1] - P[1], prev_p[4 * q + 2] - P[2]};
                    if (!(dot3(d, d) <= lim)) return;
                    acc.B = acc.B + b;
                    for (int ch = 0; ch < 3; ++ch) {
                        acc.H[ch] = std::fmaf(b, prev_c[4 * q + ch], acc.H[ch]);
                        acc.Hv[ch] = std::fmaf(b, prev_v[4 * q + ch], acc.Hv[ch]);
                    }
                    acc.HN = std::fmaf(b, prev_c[4 * q + 3], acc.HN);
                };
                if (is_static) {
                    tap(px, py, 1.0f);
                } else {
                    const Proj pr = project(M, w);
                    if (pr.ga > 0.0f) {
                        const float x = pr.x, y = pr.y;
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
                        const float h = acc.H[ch] / acc.B, hv = acc.Hv[ch] / acc.B;
                        co[ch] = std::fmaf(a, c[ch] - h, h);
                        vo[ch] = std::fmaf(a * a, s[ch], (k * k) * hv);
                    }
                    No = Ns > nm ? nm : Ns;
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

} // extern "C"
