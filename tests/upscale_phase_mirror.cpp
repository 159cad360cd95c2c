// A plain C++ restatement of guided upscaling WITH A PHASE (rayz_hip_upscaler_run_phase), written from DESIGN.md §4.20 and its
// subsection "Lattice samples"; it includes no library header and works on the caller's arrays as they are.  It is held,
// independently of the device, to the rational answers of tests/upscale_phase_cases.py, and at f = 3, phase (1, 1) to the
// restatement of the run without a phase (tests/upscale_mirror.cpp), where the two position rules coincide.  Built by
// tests/upscale_phase_cases.py with `g++ -O2 -ffp-contract=off` (an FMA happens exactly where fmaf is written).
//
// The text in short.  Full frame W x H = f·(w x h), f in 2..4, phase (px, py) with px, py < f: low-resolution pixel (i, j) IS full
// pixel (f·i + px, f·j + py).  Per pixel of either frame: index, unit normal n, point P, albedo a;  bg := index < 0;
// m_ch = demodulate && !bg ? max(a_ch, 2^-8) : 1.  Low-resolution pixel q: e_q = c_q / m_q,  ve_q,ch = clamp_var(var_q,ch /
// (m_q,ch·m_q,ch)),  clamp_var(t) = !(t < 2^32) ? 2^32 : (t > 0 ? t : 0).
//   Position of full pixel x:  a = x - px;  i0 = floor(a / f);  r = a - f·i0;  fx = f32(r) / f32(f).  Likewise y -> j0, ry, fy.
//   guide(p, q) (the guide half of §4.11's tap, centre = the full pixel, tap = the low-resolution pixel):
//       bg(p) or bg(q): not accepted unless both are background; then g = 1
//       else wn = max0(dot(n_p, n_q)), squared normal_power_log2 times;  v = P_q - P_p;  d2 = dot(v, v);  pl = dot(n_p, v)
//            wz = d2 == 0 ? 1 : u·u, u = max0(1 - (pl·pl) / (sp2·d2));  g = wn·wz
//   A SAMPLED pixel (r = 0 on both axes) whose own sample q = (i0, j0) is accepted with g > 0:  out = c_q (the raw colour, by
//     selection),  var_ch = clamp_var(var_q,ch),  stage 0.  Every other pixel:
//   Stage 0: taps (i0 + di, j0 + dj), dj outer, di inner, 0..1:  bx = di ? fx : 1 - fx, by likewise, b = bx·by;  skipped when outside
//     the low-resolution frame, when b == 0 or when not accepted;  w = b·g;  W = W + w;  acc_ch = fma(w, e_q,ch, acc_ch);
//     V_ch = fma(w·w, ve_q,ch, V_ch)
//   Stage 1, if not W >= 2^-40: sums reset, taps (i0 + di, j0 + dj), dj outer, di inner, -1..2, b = 1.
//   If W >= 2^-40: out_ch = (acc_ch / W)·m_p,ch;  var_ch = (V_ch / (W·W))·(m_p,ch·m_p,ch).
//   Stage 2 otherwise: out = c of the NEAREST sample, per axis clamp(floor((2a + f) / 2f), 0, w - 1);  var_ch = 2^32.
//   dot(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x·b.x));  max0(x) = x > 0 ? x : 0.
#include <cmath>
#include <cstddef>
#include <cstdint>

namespace {

const float CAP = 4294967296.0f;
const float LEAST_W = 1.0f / 1099511627776.0f; // 2^-40

float dot(const float* a, const float* b) { return std::fmaf(a[2], b[2], std::fmaf(a[1], b[1], a[0] * b[0])); }
float positive(float x) { return x > 0.0f ? x : 0.0f; }
float clamp_var(float t) { return !(t < CAP) ? CAP : (t > 0.0f ? t : 0.0f); }

long floored(long a, long b) { // floor(a / b), b > 0
    return a >= 0 ? a / b : -((-a + b - 1) / b);
}

struct GBuffer {
    const int32_t* index;
    const float *normal, *point, *albedo; // albedo NULL: no demodulation
    bool background(size_t p) const { return index[p] < 0; }
    float modulation(size_t p, int ch) const {
        if (!albedo || background(p)) return 1.0f;
        const float a = albedo[3 * p + ch];
        return a > 0.00390625f ? a : 0.00390625f;
    }
};

struct Problem {
    GBuffer lo, hi;
    const float *rgb_lo, *var_lo;
    long f, w, h;
    uint32_t normal_power_log2;
    float sp2;
    bool with_var;

    // whether full pixel p may be mixed with low-resolution pixel q, and with which weight
    bool guide(size_t p, size_t q, float& g) const {
        const bool bp = hi.background(p), bq = lo.background(q);
        g = 1.0f;
        if (bp || bq) return bp && bq;
        const float *np = hi.normal + 3 * p, *nq = lo.normal + 3 * q;
        float wn = positive(dot(np, nq));
        for (uint32_t k = 0; k < normal_power_log2; ++k) wn = wn * wn;
        const float v[3] = {lo.point[3 * q] - hi.point[3 * p], lo.point[3 * q + 1] - hi.point[3 * p + 1], lo.point[3 * q + 2] - hi.point[3 * p + 2]};
        const float d2 = dot(v, v), pl = dot(np, v);
        float wz = 1.0f;
        if (d2 != 0.0f) {
            const float u = positive(1.0f - (pl * pl) / (sp2 * d2));
            wz = u * u;
        }
        g = wn * wz;
        return true;
    }
};

struct Sums {
    float W = 0.0f, acc[3] = {0.0f, 0.0f, 0.0f}, V[3] = {0.0f, 0.0f, 0.0f};
    void tap(const Problem& s, size_t p, long qx, long qy, float b) {
        if (qx < 0 || qx >= s.w || qy < 0 || qy >= s.h || b == 0.0f) return;
        const size_t q = (size_t)qy * s.w + qx;
        float g;
        if (!s.guide(p, q, g)) return;
        const float wt = b * g;
        W = W + wt;
        for (int ch = 0; ch < 3; ++ch) {
            const float m = s.lo.modulation(q, ch);
            acc[ch] = std::fmaf(wt, s.rgb_lo[3 * q + ch] / m, acc[ch]);
            if (s.with_var) V[ch] = std::fmaf(wt * wt, clamp_var(s.var_lo[3 * q + ch] / (m * m)), V[ch]);
        }
    }
};

long nearest(long a, long f, long n) {
    const long i = floored(2 * a + f, 2 * f);
    return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
}

} // namespace

extern "C" {

// var_lo, var_out, stage_out may each be NULL (var_out needs var_lo).
void upscale_phase_mirror(const float* rgb_lo, const float* var_lo, const int32_t* index_lo, const float* normal_lo, const float* point_lo,
                          const float* albedo_lo, const int32_t* index_hi, const float* normal_hi, const float* point_hi,
                          const float* albedo_hi, uint32_t lo_width, uint32_t lo_height, uint32_t factor, uint32_t phase_x, uint32_t phase_y,
                          uint32_t normal_power_log2, float sp2, float* out, float* var_out, uint8_t* stage_out) {
    Problem s{{index_lo, normal_lo, point_lo, albedo_lo}, {index_hi, normal_hi, point_hi, albedo_hi}, rgb_lo, var_lo, (long)factor,
              (long)lo_width, (long)lo_height, normal_power_log2, sp2, var_lo && var_out};
    const long f = s.f, W = f * s.w, H = f * s.h;
    for (long y = 0; y < H; ++y)
        for (long x = 0; x < W; ++x) {
            const size_t p = (size_t)y * W + x;
            const long ax = x - (long)phase_x, ay = y - (long)phase_y;
            const long i0 = floored(ax, f), j0 = floored(ay, f);
            const long rx = ax - f * i0, ry = ay - f * j0;
            const float fx = (float)rx / (float)f, fy = (float)ry / (float)f;
            uint8_t stage = 0;
            if (rx == 0 && ry == 0) { // a sampled pixel: its own sample, if the guides take it
                const size_t q = (size_t)j0 * s.w + i0;
                float g;
                if (s.guide(p, q, g) && g > 0.0f) {
                    for (int ch = 0; ch < 3; ++ch) {
                        out[3 * p + ch] = rgb_lo[3 * q + ch];
                        if (s.with_var) var_out[3 * p + ch] = clamp_var(var_lo[3 * q + ch]);
                    }
                    if (stage_out) stage_out[p] = 0;
                    continue;
                }
            }
            Sums sums;
            for (long dj = 0; dj <= 1; ++dj)
                for (long di = 0; di <= 1; ++di) sums.tap(s, p, i0 + di, j0 + dj, (di ? fx : 1.0f - fx) * (dj ? fy : 1.0f - fy));
            if (!(sums.W >= LEAST_W)) {
                stage = 1;
                sums = Sums();
                for (long dj = -1; dj <= 2; ++dj)
                    for (long di = -1; di <= 2; ++di) sums.tap(s, p, i0 + di, j0 + dj, 1.0f);
            }
            if (sums.W >= LEAST_W) {
                for (int ch = 0; ch < 3; ++ch) {
                    const float m = s.hi.modulation(p, ch);
                    out[3 * p + ch] = (sums.acc[ch] / sums.W) * m;
                    if (s.with_var) var_out[3 * p + ch] = (sums.V[ch] / (sums.W * sums.W)) * (m * m);
                }
            } else {
                stage = 2;
                const size_t q = (size_t)nearest(ay, f, s.h) * s.w + (size_t)nearest(ax, f, s.w);
                for (int ch = 0; ch < 3; ++ch) {
                    out[3 * p + ch] = rgb_lo[3 * q + ch];
                    if (s.with_var) var_out[3 * p + ch] = CAP;
                }
            }
            if (stage_out) stage_out[p] = stage;
        }
}

} // extern "C"
