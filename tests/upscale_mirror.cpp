// A plain C++ restatement of guided upscaling's arithmetic contract; it includes no library header and works on the
// caller's arrays as they are (no packed records).  §4.20 fixes the order of every operation, so a restatement has the shape of the
// device's code; what makes it a check is that it is held, independently of the device, to the closed-form answers of
// tests/upscale_cases.py.  Built by tests/upscale_ref.py with `g++ -O2 -ffp-contract=off` (an FMA happens exactly where fmaf is
// written); the tests hold the GPU to it bit for bit.
//
// §4.20 in short.  Full frame W x H = f·(w x h), f in 2..4.  Per pixel of either frame: index, unit normal n, point P, albedo a;
// bg := index < 0;  m_ch = demodulate && !bg ? max(a_ch, 2^-8) : 1.  Low-resolution pixel q: e_q = c_q / m_q,
// ve_q,ch = clamp_var(var_q,ch / (m_q,ch·m_q,ch)), clamp_var(t) = !(t < 2^32) ? 2^32 : (t > 0 ? t : 0).
//   Position of full pixel x: a = 2x + 1 - f;  i0 = floor(a / 2f);  r = a - 2f·i0;  fx = f32(r) / f32(2f).  Likewise y -> j0, fy.
//   Stage 0: taps (i0 + di, j0 + dj), dj outer, di inner, 0..1:  bx = di ? fx : 1 - fx, by likewise, b = bx·by;  skipped when outside
//     the low-resolution frame or when b == 0.
//     guide weight (the guide half of §4.11's tap, centre = the full pixel, tap = the low-resolution pixel):
//       bg(p) or bg(q): skipped unless both are background; then g = 1
//       else wn = max0(dot(n_p, n_q)), squared normal_power_log2 times;  v = P_q - P_p;  d2 = dot(v, v);  pl = dot(n_p, v)
//            wz = d2 == 0 ? 1 : u·u, u = max0(1 - (pl·pl) / (sp2·d2));  g = wn·wz
//     w = b·g;  W = W + w;  acc_ch = fma(w, e_q,ch, acc_ch);  V_ch = fma(w·w, ve_q,ch, V_ch)
//   Stage 1, if not W >= 2^-40: sums reset, taps (i0 + di, j0 + dj), dj outer, di inner, -1..2, b = 1.
//   If W >= 2^-40: out_ch = (acc_ch / W)·m_p,ch;  var_ch = (V_ch / (W·W))·(m_p,ch·m_p,ch).
//   Stage 2 otherwise: out = c of low-resolution pixel (x div f, y div f), var_ch = 2^32.
//   dot(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x·b.x));  max0(x) = x > 0 ? x : 0.
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace {

const float VCAP = 4294967296.0f;
const float WMIN = 9.094947017729282e-13f; // 2^-40

inline float dot3(const float* a, const float* b) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }
inline float max0(float x) { return x > 0.0f ? x : 0.0f; }
inline float clamp_var(float t) { return !(t < VCAP) ? VCAP : (t > 0.0f ? t : 0.0f); }

inline long floor_div(long a, long b) { // b > 0
    long q = a / b;
    if (a % b != 0 && a < 0) --q;
    return q;
}

struct Frame {
    const int32_t* index;
    const float *normal, *point, *albedo; // albedo NULL: m = 1
    void modulation(size_t p, float m[3]) const {
        m[0] = m[1] = m[2] = 1.0f;
        if (albedo && index[p] >= 0)
            for (int c = 0; c < 3; ++c) m[c] = albedo[3 * p + c] > 0.00390625f ? albedo[3 * p + c] : 0.00390625f;
    }
};

struct Sums {
    float W, acc[3], V[3];
};

} // namespace

extern "C" {

// var_lo, var_out, stage_out may each be NULL (var_out needs var_lo).
void upscale_mirror(const float* rgb_lo, const float* var_lo, const int32_t* index_lo, const float* normal_lo, const float* point_lo,
                    const float* albedo_lo, const int32_t* index_hi, const float* normal_hi, const float* point_hi, const float* albedo_hi,
                    uint32_t lo_width, uint32_t lo_height, uint32_t factor, uint32_t normal_power_log2, float sp2, float* out, float* var_out,
                    uint8_t* stage_out) {
    const long f = factor, w = lo_width, h = lo_height, Wf = f * w, Hf = f * h;
    const Frame lo{index_lo, normal_lo, point_lo, albedo_lo}, hi{index_hi, normal_hi, point_hi, albedo_hi};
    const bool with_var = var_lo && var_out;
    for (long y = 0; y < Hf; ++y)
        for (long x = 0; x < Wf; ++x) {
            const size_t p = (size_t)y * Wf + x;
            const bool bgp = hi.index[p] < 0;
            const float *np = hi.normal + 3 * p, *Pp = hi.point + 3 * p;
            float mp[3];
            hi.modulation(p, mp);
            const long ax = 2 * x + 1 - f, ay = 2 * y + 1 - f;
            const long i0 = floor_div(ax, 2 * f), j0 = floor_div(ay, 2 * f);
            const float fx = (float)(ax - 2 * f * i0) / (float)(2 * f), fy = (float)(ay - 2 * f * j0) / (float)(2 * f);
            Sums s;
            int stage = 0;
            for (; stage < 2; ++stage) {
                s = Sums{0.0f, {0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f}};
                const long d0 = stage ? -1 : 0, d1 = stage ? 2 : 1;
                for (long dj = d0; dj <= d1; ++dj)
                    for (long di = d0; di <= d1; ++di) {
                        const long qx = i0 + di, qy = j0 + dj;
                        float b = 1.0f;
                        if (stage == 0) {
                            const float bx = di ? fx : 1.0f - fx, by = dj ? fy : 1.0f - fy;
                            b = bx * by;
                        }
                        if (qx < 0 || qx >= w || qy < 0 || qy >= h) continue;
                        if (b == 0.0f) continue;
                        const size_t q = (size_t)qy * w + qx;
                        const bool bgq = lo.index[q] < 0;
                        const float *nq = lo.normal + 3 * q, *Pq = lo.point + 3 * q;
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
                        float mq[3];
                        lo.modulation(q, mq);
                        const float wt = b * g;
                        s.W = s.W + wt;
                        for (int c = 0; c < 3; ++c) {
                            s.acc[c] = std::fmaf(wt, rgb_lo[3 * q + c] / mq[c], s.acc[c]);
                            if (with_var) s.V[c] = std::fmaf(wt * wt, clamp_var(var_lo[3 * q + c] / (mq[c] * mq[c])), s.V[c]);
                        }
                    }
                if (s.W >= WMIN) break;
            }
            if (stage < 2) {
                for (int c = 0; c < 3; ++c) {
                    out[3 * p + c] = (s.acc[c] / s.W) * mp[c];
                    if (with_var) var_out[3 * p + c] = (s.V[c] / (s.W * s.W)) * (mp[c] * mp[c]);
                }
            } else {
                const size_t q = (size_t)(y / f) * w + (size_t)(x / f);
                for (int c = 0; c < 3; ++c) {
                    out[3 * p + c] = rgb_lo[3 * q + c];
                    if (with_var) var_out[3 * p + c] = VCAP;
                }
            }
            if (stage_out) stage_out[p] = (uint8_t)stage;
        }
}

} // extern "C"
