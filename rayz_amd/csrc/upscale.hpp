// upscale.hpp — guided upscaling's device code (include/rayz_hip.h: rayz_hip_upscaler_*).
//
// A frame traced at 1/f of the resolution in each direction is rebuilt at full size under a full-size G-buffer: the low-resolution
// frame is packed ONCE into the denoiser's 16-byte records (denoise_pack_kernel as it stands: guides, modulation m, demodulated
// colour e = c / m) plus, when the caller has a variance, a record of the per-channel demodulated variance; then ONE launch, a
// thread per full pixel, weighs the 2x2 low-resolution pixels around it by their bilinear weight times the guide weight of the
// à-trous tap (dn_guide(), shared with the denoiser: the full pixel's guides are the centre, the low-resolution pixel's the tap),
// and multiplies the full pixel's own modulation back in — texture detail comes from the full-size albedo, only the irradiance
// is interpolated.  A pixel no tap of its 2x2 footprint may be mixed with (W < 2^-40: a thin feature, a silhouette) tries the 4x4
// footprint with the guide weight alone, and failing that takes the nearest low-resolution pixel's raw colour.
//
// The arithmetic is a contract (§4.20): + - x, the FMAs written below, correctly rounded divides, comparisons, integer
// arithmetic — restated bit for bit by tests/upscale_mirror.cpp.  The full-size guides are read straight from the caller's
// G-buffer, once each; the low-resolution records come through L1 / L2 (a 32x8 tile touches at most (32/f + 2) x (8/f + 2) of them).
#pragma once

#include "denoise.hpp"

namespace rayz_dev {

struct UpscaleArgs {
    const dn4* __restrict__ ga;   // low resolution, per pixel {n.x, n.y, n.z, bg ? 1 : 0}
    const dn4* __restrict__ gb;   // .. {P.x, P.y, P.z, 0}
    const dn4* __restrict__ col;  // .. {e.r, e.g, e.b, 0}
    const dn4* __restrict__ var;  // .. {ve.r, ve.g, ve.b, 0} (VAR only)
    const float* __restrict__ rgb_lo;   // the caller's low-resolution frame: stage 2's raw colour
    const int32_t* __restrict__ index;  // the full-size G-buffer
    const float* __restrict__ normal;
    const float* __restrict__ point;
    const float* __restrict__ albedo;   // NULL: m = 1
    float* __restrict__ rgb;            // full-size packed RGB out
    float* __restrict__ var_out;        // full-size per-channel variance out (VAR only)
    uint8_t* __restrict__ stage;        // full-size stage map out, or NULL
    uint32_t width, height;             // the full frame, = factor x (lo_width, lo_height)
    uint32_t lo_width, lo_height;
    uint32_t factor;
    uint32_t normal_power_log2;
    float sp2;                          // f32(sigma_plane) x f32(sigma_plane)
};

struct UpAcc {
    float W, r, g, b, vr, vg, vb;
};

// A stage is taken only with W >= 2^-40 (§4.20): the largest of its at most 16 weights is then at least 2^-44, so neither its
// square nor W·W underflows in f32.  With "W > 0" a footprint of nearly refused taps (cos^64 at a sphere's limb) gave V = W·W = 0
// and a NaN variance.
constexpr float kUpMinW = 0x1p-40f;

// The per-channel variance record of the low-resolution frame: ve_ch = clamp_var(var_ch / (m_ch·m_ch)) with the pack pass's m.
__global__ __launch_bounds__(256) void upscale_pack_var_kernel(const float* __restrict__ var_rgb, const dn4* __restrict__ mod,
                                                               dn4* __restrict__ var, size_t n_pixels) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pixels) return;
    const dn4 m = mod[p];
    var[p] = dn4{dn_clamp_var(var_rgb[3 * p] / (m.x * m.x)), dn_clamp_var(var_rgb[3 * p + 1] / (m.y * m.y)),
                 dn_clamp_var(var_rgb[3 * p + 2] / (m.z * m.z)), 0.0f};
}

// One tap: low-resolution pixel (qx, qy), inside the frame, with the position weight b.
template <bool VAR>
__device__ __forceinline__ void up_tap(const UpscaleArgs& a, const dn4 pa, const dn4 pb, const int qx, const int qy, const float b, UpAcc& acc) {
    const size_t q = (size_t)qy * a.lo_width + qx;
    const dn4 qa = a.ga[q], qb = a.gb[q];
    float g;
    if (!dn_guide(pa, pb, qa, qb, a.normal_power_log2, a.sp2, g)) return;
    const dn4 qc = a.col[q];
    const float w = b * g;
    acc.W = acc.W + w;
    acc.r = __builtin_fmaf(w, qc.x, acc.r);
    acc.g = __builtin_fmaf(w, qc.y, acc.g);
    acc.b = __builtin_fmaf(w, qc.z, acc.b);
    if (VAR) {
        const dn4 qv = a.var[q];
        const float w2 = w * w;
        acc.vr = __builtin_fmaf(w2, qv.x, acc.vr);
        acc.vg = __builtin_fmaf(w2, qv.y, acc.vg);
        acc.vb = __builtin_fmaf(w2, qv.z, acc.vb);
    }
}

// §4.20's position along one axis: a = 2x + 1 - f, i0 = floor(a / 2f), fx = f32(a - 2f·i0) / f32(2f).  (a > -2f: i0 >= -1)
__device__ __forceinline__ void up_position(const int x, const int f, int& i0, float& fx) {
    const int a = 2 * x + 1 - f;
    i0 = a < 0 ? -1 : a / (2 * f);
    fx = (float)(a - 2 * f * i0) / (float)(2 * f);
}

// One full pixel per thread, 32x8 tiles.
template <bool VAR> __global__ __launch_bounds__(256) void upscale_direct_kernel(const UpscaleArgs a) {
    const int x = (int)(blockIdx.x * kDnTileW + threadIdx.x % kDnTileW);
    const int y = (int)(blockIdx.y * kDnTileH + threadIdx.x / kDnTileW);
    if (x >= (int)a.width || y >= (int)a.height) return;
    const size_t p = (size_t)y * a.width + x;
    const bool bg = a.index[p] < 0;
    const dn4 pa{a.normal[3 * p], a.normal[3 * p + 1], a.normal[3 * p + 2], bg ? 1.0f : 0.0f};
    const dn4 pb{a.point[3 * p], a.point[3 * p + 1], a.point[3 * p + 2], 0.0f};
    float mr = 1.0f, mg = 1.0f, mb = 1.0f;
    if (a.albedo && !bg) { // the pack pass's modulation, of the FULL pixel
        const float lo = 0.00390625f; // 2^-8
        const float ar = a.albedo[3 * p], ag = a.albedo[3 * p + 1], ab = a.albedo[3 * p + 2];
        mr = ar > lo ? ar : lo;
        mg = ag > lo ? ag : lo;
        mb = ab > lo ? ab : lo;
    }
    const int f = (int)a.factor, w = (int)a.lo_width, h = (int)a.lo_height;
    int i0, j0;
    float fx, fy;
    up_position(x, f, i0, fx);
    up_position(y, f, j0, fy);
    UpAcc acc{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t stage = 0;
    // stage 0: the 2x2 footprint, bilinear weight x guide weight
#pragma unroll
    for (int dj = 0; dj < 2; ++dj) {
        const int qy = j0 + dj;
        const float by = dj ? fy : 1.0f - fy;
#pragma unroll
        for (int di = 0; di < 2; ++di) {
            const int qx = i0 + di;
            const float b = (di ? fx : 1.0f - fx) * by;
            if (qx < 0 || qx >= w || qy < 0 || qy >= h || b == 0.0f) continue;
            up_tap<VAR>(a, pa, pb, qx, qy, b, acc);
        }
    }
    if (!(acc.W >= kUpMinW)) { // stage 1 (rare): the 4x4 footprint, guide weight alone
        stage = 1;
        acc = UpAcc{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int dj = -1; dj <= 2; ++dj) {
            const int qy = j0 + dj;
            if (qy < 0 || qy >= h) continue;
            for (int di = -1; di <= 2; ++di) {
                const int qx = i0 + di;
                if (qx < 0 || qx >= w) continue;
                up_tap<VAR>(a, pa, pb, qx, qy, 1.0f, acc);
            }
        }
    }
    if (acc.W >= kUpMinW) {
        a.rgb[3 * p + 0] = (acc.r / acc.W) * mr;
        a.rgb[3 * p + 1] = (acc.g / acc.W) * mg;
        a.rgb[3 * p + 2] = (acc.b / acc.W) * mb;
        if (VAR) {
            const float W2 = acc.W * acc.W;
            a.var_out[3 * p + 0] = (acc.vr / W2) * (mr * mr);
            a.var_out[3 * p + 1] = (acc.vg / W2) * (mg * mg);
            a.var_out[3 * p + 2] = (acc.vb / W2) * (mb * mb);
        }
    } else { // stage 2: the nearest low-resolution pixel's raw colour, and "no estimate" as its variance
        stage = 2;
        const size_t q = (size_t)(y / f) * a.lo_width + (size_t)(x / f);
        a.rgb[3 * p + 0] = a.rgb_lo[3 * q + 0];
        a.rgb[3 * p + 1] = a.rgb_lo[3 * q + 1];
        a.rgb[3 * p + 2] = a.rgb_lo[3 * q + 2];
        if (VAR) a.var_out[3 * p + 0] = a.var_out[3 * p + 1] = a.var_out[3 * p + 2] = kDnVarCap;
    }
    if (a.stage) a.stage[p] = (uint8_t)stage;
}

// ---- the run with a phase (§4.20, "Lattice samples"; rayz_hip_upscaler_run_phase) -----------------------------------------------
// Low-resolution pixel (i, j) IS full pixel (f·i + phase_x, f·j + phase_y): a sample of a lattice, not the mean of a block.  A
// sibling of upscale_direct_kernel — its text repeated with the position, the nearest sample and the pass-through of a sampled
// pixel replaced — so that the kernel above stays the kernel it was; up_tap and dn_guide are shared.
struct UpscalePhaseArgs {
    UpscaleArgs a;
    const float* __restrict__ var_lo; // the caller's low-resolution variance: a sampled pixel's raw variance (VAR only)
    uint32_t phase_x, phase_y;
};

// The position along one axis: a = x - phase, i0 = floor(a / f), r = a - f·i0, fx = f32(r) / f32(f).  (a > -f: i0 >= -1)
__device__ __forceinline__ void up_phase_position(const int x, const int phase, const int f, int& i0, int& r, float& fx) {
    const int a = x - phase;
    i0 = a < 0 ? -1 : a / f;
    r = a - f * i0;
    fx = (float)r / (float)f;
}

// The nearest sample along one axis: clamp(floor((2a + f) / 2f), 0, n - 1).
__device__ __forceinline__ int up_phase_nearest(const int x, const int phase, const int f, const int n) {
    const int t = 2 * (x - phase) + f;
    const int i = t < 0 ? 0 : t / (2 * f);
    return i < n ? i : n - 1;
}

template <bool VAR> __global__ __launch_bounds__(256) void upscale_phase_kernel(const UpscalePhaseArgs pa_) {
    const UpscaleArgs& a = pa_.a;
    const int x = (int)(blockIdx.x * kDnTileW + threadIdx.x % kDnTileW);
    const int y = (int)(blockIdx.y * kDnTileH + threadIdx.x / kDnTileW);
    if (x >= (int)a.width || y >= (int)a.height) return;
    const size_t p = (size_t)y * a.width + x;
    const bool bg = a.index[p] < 0;
    const dn4 pa{a.normal[3 * p], a.normal[3 * p + 1], a.normal[3 * p + 2], bg ? 1.0f : 0.0f};
    const dn4 pb{a.point[3 * p], a.point[3 * p + 1], a.point[3 * p + 2], 0.0f};
    const int f = (int)a.factor, w = (int)a.lo_width, h = (int)a.lo_height;
    int i0, j0, rx, ry;
    float fx, fy;
    up_phase_position(x, (int)pa_.phase_x, f, i0, rx, fx);
    up_phase_position(y, (int)pa_.phase_y, f, j0, ry, fy);
    if (rx == 0 && ry == 0 && i0 < w && j0 < h) { // a SAMPLED pixel (i0, j0 >= 0 here): its own sample passes through, by selection
        const size_t q = (size_t)j0 * a.lo_width + i0;
        float g;
        if (dn_guide(pa, pb, a.ga[q], a.gb[q], a.normal_power_log2, a.sp2, g) && g > 0.0f) {
            a.rgb[3 * p + 0] = a.rgb_lo[3 * q + 0];
            a.rgb[3 * p + 1] = a.rgb_lo[3 * q + 1];
            a.rgb[3 * p + 2] = a.rgb_lo[3 * q + 2];
            if (VAR) {
                a.var_out[3 * p + 0] = dn_clamp_var(pa_.var_lo[3 * q + 0]);
                a.var_out[3 * p + 1] = dn_clamp_var(pa_.var_lo[3 * q + 1]);
                a.var_out[3 * p + 2] = dn_clamp_var(pa_.var_lo[3 * q + 2]);
            }
            if (a.stage) a.stage[p] = 0;
            return;
        }
    }
    float mr = 1.0f, mg = 1.0f, mb = 1.0f;
    if (a.albedo && !bg) { // the pack pass's modulation, of the FULL pixel
        const float lo = 0.00390625f; // 2^-8
        const float ar = a.albedo[3 * p], ag = a.albedo[3 * p + 1], ab = a.albedo[3 * p + 2];
        mr = ar > lo ? ar : lo;
        mg = ag > lo ? ag : lo;
        mb = ab > lo ? ab : lo;
    }
    UpAcc acc{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    uint32_t stage = 0;
    // stage 0: the 2x2 footprint, bilinear weight x guide weight
#pragma unroll
    for (int dj = 0; dj < 2; ++dj) {
        const int qy = j0 + dj;
        const float by = dj ? fy : 1.0f - fy;
#pragma unroll
        for (int di = 0; di < 2; ++di) {
            const int qx = i0 + di;
            const float b = (di ? fx : 1.0f - fx) * by;
            if (qx < 0 || qx >= w || qy < 0 || qy >= h || b == 0.0f) continue;
            up_tap<VAR>(a, pa, pb, qx, qy, b, acc);
        }
    }
    if (!(acc.W >= kUpMinW)) { // stage 1 (rare): the 4x4 footprint, guide weight alone
        stage = 1;
        acc = UpAcc{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int dj = -1; dj <= 2; ++dj) {
            const int qy = j0 + dj;
            if (qy < 0 || qy >= h) continue;
            for (int di = -1; di <= 2; ++di) {
                const int qx = i0 + di;
                if (qx < 0 || qx >= w) continue;
                up_tap<VAR>(a, pa, pb, qx, qy, 1.0f, acc);
            }
        }
    }
    if (acc.W >= kUpMinW) {
        a.rgb[3 * p + 0] = (acc.r / acc.W) * mr;
        a.rgb[3 * p + 1] = (acc.g / acc.W) * mg;
        a.rgb[3 * p + 2] = (acc.b / acc.W) * mb;
        if (VAR) {
            const float W2 = acc.W * acc.W;
            a.var_out[3 * p + 0] = (acc.vr / W2) * (mr * mr);
            a.var_out[3 * p + 1] = (acc.vg / W2) * (mg * mg);
            a.var_out[3 * p + 2] = (acc.vb / W2) * (mb * mb);
        }
    } else { // stage 2: the nearest sample's raw colour, and "no estimate" as its variance
        stage = 2;
        const size_t q = (size_t)up_phase_nearest(y, (int)pa_.phase_y, f, h) * a.lo_width + (size_t)up_phase_nearest(x, (int)pa_.phase_x, f, w);
        a.rgb[3 * p + 0] = a.rgb_lo[3 * q + 0];
        a.rgb[3 * p + 1] = a.rgb_lo[3 * q + 1];
        a.rgb[3 * p + 2] = a.rgb_lo[3 * q + 2];
        if (VAR) a.var_out[3 * p + 0] = a.var_out[3 * p + 1] = a.var_out[3 * p + 2] = kDnVarCap;
    }
    if (a.stage) a.stage[p] = (uint8_t)stage;
}

// ---- host side: the launches (upscaler.hpp owns the handle, the validation and the stream) --------------------------------------
inline void upscale_launch_phase(hipStream_t st, bool with_var, const UpscalePhaseArgs& a) {
    hipLaunchKernelGGL(with_var ? upscale_phase_kernel<true> : upscale_phase_kernel<false>, denoise_grid(a.a.width, a.a.height), dim3(256), 0, st, a);
}

inline void upscale_launch_pack_var(hipStream_t st, const float* var_rgb, const dn4* mod, dn4* var, size_t n_pixels) {
    hipLaunchKernelGGL(upscale_pack_var_kernel, dim3((uint32_t)((n_pixels + 255) / 256)), dim3(256), 0, st, var_rgb, mod, var, n_pixels);
}

inline void upscale_launch(hipStream_t st, bool with_var, const UpscaleArgs& a) {
    hipLaunchKernelGGL(with_var ? upscale_direct_kernel<true> : upscale_direct_kernel<false>, denoise_grid(a.width, a.height), dim3(256), 0, st, a);
}

} // namespace rayz_dev
