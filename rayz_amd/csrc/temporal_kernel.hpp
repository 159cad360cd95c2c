// temporal_kernel.hpp — temporal accumulation's device code (include/rayz_hip.h: rayz_hip_temporal_*; the handle,
// the host part of a step and the validation: temporal.hpp).
//
// ONE launch per step: every pixel of the current frame finds where its first-hit point lay in the previous frame, gathers the four
// history pixels around that position, keeps the ones that are the same surface, blends the current sample into their
// interpolated mean by sample count and writes the new history, the blended colour and its variance.  A gather-and-stream kernel:
// per pixel it reads 52 bytes of the caller's frame (colour, variance, index, normal, point) and one history record of 4 x 16 B,
// and writes one history record and 24 (28 with the length) bytes; the other three taps of a pixel are its neighbours' compulsory
// reads, which is why pixels are dealt as the denoiser's 32x8 tiles — a wave covers two rows of 32 pixels, and for a pan of a few
// pixels its taps fall in the 33x3 records around them, 16-byte records in four arrays read and written as dwordx4.  No LDS: a tap's
// position is data-dependent, and a tile's taps need not lie in a tile.
//
// The arithmetic is a contract (§4.15): + - x, the FMAs written below, correctly rounded divides, floor, comparisons — so that
// tests/temporal_mirror.cpp restates it bit for bit.  What a tap decides is in ta_accepts(), what it adds in TaAcc::add(); the static
// form (the camera did not move: the one tap is the pixel's own record) is a template flag of the same kernel.
//
// ta_gather() is the single statement of §4.15 steps 1-4 up to the sums for all three modes — the reprojection through M, the
// tap positions and weights, the two rounds of loads, the acceptance, the sums in tap order — and ta_blend_head() / ta_blend()
// that of the blend weight, the capped length and the blend itself: the moments and the feedback step (§4.16, §4.17;
// temporal_moments_kernel.hpp, temporal_feedback_kernel.hpp) call them with their own record lists and blend their own channels.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include <type_traits>

#include "denoise.hpp" // dn4, dn_dot, dn_clamp_var, the tile and its grid

namespace rayz_dev {

constexpr float kTaMinWeight = 0.015625f; // 2^-6: below this accepted bilinear weight there is no history

struct TemporalHistory { // four arrays of one 16-byte record per pixel
    dn4* c; // {c.r, c.g, c.b, N}: accumulated radiance, history length in samples
    dn4* v; // {v.r, v.g, v.b, 0}: variance of that mean
    dn4* g; // {n.x, n.y, n.z, bits(index)}
    dn4* p; // {P.x, P.y, P.z, 0}
};

struct TemporalArgs {
    const float* rgb;                  // the current frame, packed RGB (may be rgb_out: a pixel reads only its own)
    const float* var;                  // its per-channel variance (may be var_out)
    const int32_t* __restrict__ index; // the current frame's guides
    const float* __restrict__ normal;
    const float* __restrict__ point;
    TemporalHistory prev, next;        // ping-pong: never the same buffer
    float* rgb_out;
    float* var_out;
    float* len_out;                    // or NULL
    uint32_t width, height;
    uint32_t has_history;
    float M[9];                        // the PREVIOUS camera's: rows (v×a)/det, (a×u)/det, (u×v)/det
    float from[3];                     // the previous camera's look_from
    float spp, am, nm, cm, r2;         // f32 of samples per pixel, alpha_min, n_max, normal_cos_min; r2 = f32(max_rel_dist)²
};

// A tap's guide records against the current pixel's id, n, P and lim = r2·|P − from|²: is this history pixel the same surface?
__device__ __forceinline__ bool ta_accepts(const TemporalArgs& a, const dn4 g, const dn4 pp, int32_t id, float nx, float ny, float nz,
                                           float Px, float Py, float Pz, float lim) {
    if (__float_as_int(g.w) != id) return false;
    if (!(dn_dot(g.x, g.y, g.z, nx, ny, nz) >= a.cm)) return false;
    const float dx = pp.x - Px, dy = pp.y - Py, dz = pp.z - Pz;
    return dn_dot(dx, dy, dz, dx, dy, dz) <= lim;
}

// The sums over a pixel's accepted taps: their bilinear weights and, for each of the R records a tap adds, the weighted records.
// The plain step adds {c, v}, the moments step {c, m}, the feedback step {c, m, m1}; record 0 is always c, whose .w is the length.
// (A lane no mode reads — the .w of v and of m1 — is summed here and dropped by the compiler: it costs no instruction.)
template <int R> struct TaAcc {
    float B = 0.0f;
    float sum[R][4] = {};

    // An accepted tap of bilinear weight b joins the sums.  Only the order of TAPS within one sum is the contract; the sums of
    // different records and lanes are independent of each other.
    __device__ __forceinline__ void add(const dn4 (&rec)[R], float b) {
        B = B + b;
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < R; ++r) sum[r][j] = __builtin_fmaf(b, rec[r][j], sum[r][j]);
    }
    __device__ __forceinline__ bool found() const { return B >= kTaMinWeight; } // else there is no history: step 4's selection
    __device__ __forceinline__ float mean(int r, int j) const { return sum[r][j] / B; }
};

// What ta_gather's moving form leaves behind for §4.26 (temporal_cubic_kernel.hpp), where a caller asks for it: the tap position
// and its fractions, lim, and each of the four taps' verdict and records.  Set where the projection passed (so wherever found()).
template <int R> struct TaTaps {
    int ix, iy;
    float fx, fy, lim;
    bool ok[4];
    dn4 tap[4][R];
};
struct TaNoTaps {}; // nothing is kept: every step but the cubic ones

// §4.15 steps 1-3 for one pixel with id >= 0 of a handle with history: the sums over the history taps that are the same surface.
// rec: the R arrays of the previous side whose records an accepted tap adds.  STATIC (the camera did not move): the one tap is
// the pixel's own record, with weight 1.  LIVE (the counts step, §4.23): a tap is also refused where its record's length is not > 0 —
// a record that holds no samples; the plain, moments and feedback steps never write one and compile without the test.
// keep: where the moving form leaves its taps (a TaTaps<R>*), or nothing.
template <bool STATIC, int R, bool LIVE = false, class Keep = TaNoTaps>
__device__ __forceinline__ TaAcc<R> ta_gather(const TemporalArgs& a, const dn4* const* rec, size_t p, int32_t id, float nx, float ny,
                                              float nz, float Px, float Py, float Pz, [[maybe_unused]] Keep* keep = nullptr) {
    TaAcc<R> acc;
    const float wx = Px - a.from[0], wy = Py - a.from[1], wz = Pz - a.from[2];
    const float lim = a.r2 * dn_dot(wx, wy, wz, wx, wy, wz);
    if (STATIC) {
        if (ta_accepts(a, a.prev.g[p], a.prev.p[p], id, nx, ny, nz, Px, Py, Pz, lim)) {
            dn4 own[R];
#pragma unroll
            for (int r = 0; r < R; ++r) own[r] = rec[r][p];
            if (!LIVE || own[0].w > 0.0f) acc.add(own, 1.0f);
        }
        return acc;
    }
    const float al = __builtin_fmaf(a.M[2], wz, __builtin_fmaf(a.M[1], wy, a.M[0] * wx));
    const float be = __builtin_fmaf(a.M[5], wz, __builtin_fmaf(a.M[4], wy, a.M[3] * wx));
    const float ga = __builtin_fmaf(a.M[8], wz, __builtin_fmaf(a.M[7], wy, a.M[6] * wx));
    if (!(ga > 0.0f)) return acc;
    const float hx = al / ga, hy = be / ga;
    if (!(hx > -1.0f && hx < (float)a.width && hy > -1.0f && hy < (float)a.height)) return acc; // (so the casts below are in range)
    const float x0 = __builtin_floorf(hx), y0 = __builtin_floorf(hy);
    const float fx = hx - x0, fy = hy - y0;
    const int ix = (int)x0, iy = (int)y0;
    // The four taps in two rounds of loads, so that a pixel waits for memory twice and not once per record: first every tap's
    // guide records, then the records it adds.  A tap outside the frame loads the nearest pixel inside it (a valid address) and
    // is refused; a refused tap's records are loaded and not used.
    size_t q[4];
    bool ok[4];
    dn4 g[4], pp[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int qx = ix + (t & 1), qy = iy + (t >> 1);
        ok[t] = qx >= 0 && qx < (int)a.width && qy >= 0 && qy < (int)a.height;
        const int cx = qx < 0 ? 0 : (qx >= (int)a.width ? (int)a.width - 1 : qx);
        const int cy = qy < 0 ? 0 : (qy >= (int)a.height ? (int)a.height - 1 : qy);
        q[t] = (size_t)cy * a.width + (size_t)cx;
        g[t] = a.prev.g[q[t]], pp[t] = a.prev.p[q[t]];
    }
    dn4 tap[4][R];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        ok[t] = ok[t] && ta_accepts(a, g[t], pp[t], id, nx, ny, nz, Px, Py, Pz, lim);
#pragma unroll
        for (int r = 0; r < R; ++r) tap[t][r] = rec[r][q[t]];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) // j outer, i inner: t = 2·j + i
        if (ok[t] && (!LIVE || tap[t][0].w > 0.0f)) acc.add(tap[t], ((t & 1) ? fx : 1.0f - fx) * ((t >> 1) ? fy : 1.0f - fy));
    if constexpr (!std::is_same<Keep, TaNoTaps>::value) {
        keep->ix = ix, keep->iy = iy, keep->fx = fx, keep->fy = fy, keep->lim = lim;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            keep->ok[t] = ok[t];
#pragma unroll
            for (int r = 0; r < R; ++r) keep->tap[t][r] = tap[t][r];
        }
    }
    return acc;
}

// §4.15 step 4's head, from the sums of a pixel that found history: the blend weight al, k = 1 − al and the capped new length.
struct TaBlend {
    float al, k, N;
};

// spp: the samples the current frame adds to this pixel — the step's one count, or in the counts step (§4.23) the pixel's own.
template <int R> __device__ __forceinline__ TaBlend ta_blend_head(const TaAcc<R>& acc, const TemporalArgs& a, float spp) {
    const float hN = acc.mean(0, 3);
    const float Ns = hN + spp;
    const float a0 = spp / Ns;
    const float al = a0 < a.am ? a.am : a0;
    return TaBlend{al, 1.0f - al, Ns > a.nm ? a.nm : Ns};
}

template <int R> __device__ __forceinline__ TaBlend ta_blend_head(const TaAcc<R>& acc, const TemporalArgs& a) {
    return ta_blend_head(acc, a, a.spp);
}

// .. and the blend of the current frame's x into the history's h, which the colour, m1 and m2 channels share.
__device__ __forceinline__ float ta_blend(float al, float x, float h) { return __builtin_fmaf(al, x - h, h); }

template <bool STATIC> __global__ __launch_bounds__(256) void temporal_step_kernel(const TemporalArgs a) {
    const int x = (int)(blockIdx.x * kDnTileW + threadIdx.x % kDnTileW);
    const int y = (int)(blockIdx.y * kDnTileH + threadIdx.x / kDnTileW);
    if (x >= (int)a.width || y >= (int)a.height) return;
    const size_t p = (size_t)y * a.width + (size_t)x;
    const float cr = a.rgb[3 * p], cg = a.rgb[3 * p + 1], cb = a.rgb[3 * p + 2];
    const float sr = dn_clamp_var(a.var[3 * p]), sg = dn_clamp_var(a.var[3 * p + 1]), sb = dn_clamp_var(a.var[3 * p + 2]);
    const int32_t id = a.index[p];
    const float nx = a.normal[3 * p], ny = a.normal[3 * p + 1], nz = a.normal[3 * p + 2];
    const float Px = a.point[3 * p], Py = a.point[3 * p + 1], Pz = a.point[3 * p + 2];
    float or_ = cr, og = cg, ob = cb, vr = sr, vg = sg, vb = sb, No = a.spp; // no history: the input, by selection
    if (id >= 0 && a.has_history) {
        const dn4* const rec[2] = {a.prev.c, a.prev.v};
        const TaAcc<2> acc = ta_gather<STATIC, 2>(a, rec, p, id, nx, ny, nz, Px, Py, Pz);
        if (acc.found()) {
            const TaBlend h = ta_blend_head(acc, a);
            const float a2 = h.al * h.al, k2 = h.k * h.k;
            or_ = ta_blend(h.al, cr, acc.mean(0, 0));
            og = ta_blend(h.al, cg, acc.mean(0, 1));
            ob = ta_blend(h.al, cb, acc.mean(0, 2));
            vr = __builtin_fmaf(a2, sr, k2 * acc.mean(1, 0));
            vg = __builtin_fmaf(a2, sg, k2 * acc.mean(1, 1));
            vb = __builtin_fmaf(a2, sb, k2 * acc.mean(1, 2));
            No = h.N;
        }
    }
    a.next.c[p] = dn4{or_, og, ob, No};
    a.next.v[p] = dn4{vr, vg, vb, 0.0f};
    a.next.g[p] = dn4{nx, ny, nz, __int_as_float(id)};
    a.next.p[p] = dn4{Px, Py, Pz, 0.0f};
    a.rgb_out[3 * p] = or_, a.rgb_out[3 * p + 1] = og, a.rgb_out[3 * p + 2] = ob;
    a.var_out[3 * p] = vr, a.var_out[3 * p + 1] = vg, a.var_out[3 * p + 2] = vb;
    if (a.len_out) a.len_out[p] = No;
}

// ---- host side: the launch of any of the three modes' steps (temporal.hpp owns the handle, the validation and the stream) ------
// still, moving: the <true> and <false> instantiations of a step kernel template.
template <class Args>
inline void temporal_launch_step(hipStream_t st, void (*still)(Args), void (*moving)(Args), bool is_static, const Args& a, uint32_t width,
                                 uint32_t height) {
    hipLaunchKernelGGL(is_static ? still : moving, denoise_grid(width, height), dim3(256), 0, st, a);
}

} // namespace rayz_dev
