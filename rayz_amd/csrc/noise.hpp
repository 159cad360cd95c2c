// noise.hpp — the progressive renderer's noise estimate (include/rayz_hip.h: rayz_hip_progressive_noise,
// _run_until, rayz_hip_noise_kat).
//
// The chunk sums of one pixel are independent sums of iid samples; their spread estimates the variance of the pixel's mean.
// A tracked handle keeps, beside the accumulator, Q_ch = Σ_k S_k,ch² / n_k per pixel (f64, one 32-byte record), folded in chunk
// order by accumulate_moments_kernel — the tracked form of accumulate_kernel: the same `acc` additions in the same order, so no
// image changes.  noise_eval_kernel turns (acc, Q, K chunks, N samples) into the per-pixel variance of the mean and its square
// relative to the pixel's brightness, and reduces three summary values.
//
// The arithmetic is a contract (§4.12): f64, + - x / only, correctly rounded, no FMA (the library is built with
// -ffp-contract=off), comparisons; no sqrt.  tests/noise_ref.py restates it in numpy bit for bit.  Everything a pixel computes
// is in nz_fold() and nz_eval(): the kernels and rayz_hip_noise_kat run the same code.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "device_types.hpp"

namespace rayz_dev {

// Q = Q + (t · t) / n for chunk sum s (widened exactly) of n samples.
template <class R> __device__ __forceinline__ void nz_fold(double& Q, const R s, const double n) {
    const double t = (double)s;
    Q = Q + (t * t) / n;
}

struct NzEval {
    double var, rel2; // variance of the pixel mean (channels summed); var / max(|mean|², floor2)
};

// K chunks and N samples done (as doubles: both are exact), M = f64(acc).  K < 2: no estimate yet, +inf.
__device__ __forceinline__ NzEval nz_eval(const double Mr, const double Mg, const double Mb, const double Qr, const double Qg,
                                          const double Qb, const double K, const double N, const double floor2) {
    NzEval e;
    if (K < 2.0) {
        e.var = e.rel2 = __builtin_inf();
        return e;
    }
    double Dr = Qr - (Mr * Mr) / N, Dg = Qg - (Mg * Mg) / N, Db = Qb - (Mb * Mb) / N;
    Dr = Dr < 0.0 ? 0.0 : Dr; // (a NaN stays a NaN)
    Dg = Dg < 0.0 ? 0.0 : Dg;
    Db = Db < 0.0 ? 0.0 : Db;
    e.var = ((Dr + Dg) + Db) / ((K - 1.0) * N);
    const double m2 = ((Mr * Mr + Mg * Mg) + Mb * Mb) / (N * N);
    const double den = m2 > floor2 ? m2 : floor2;
    e.rel2 = e.var / den;
    return e;
}

// ---- the tracked fold: acc = acc + partial[k], Q = Q + partial[k]² / n_k for the pass's chunks in chunk order -----------------
// accumulate_kernel plus the moments.  `sizes` points at the schedule entry of the pass's first chunk (starts + c0): chunk k of
// the pass holds sizes[k + 1] - sizes[k] samples (wave-uniform: scalar loads).  Streaming: one 16-byte (f32) or 32-byte (f64)
// load per chunk and pixel; acc and the 32-byte Q record are read (not by the first pass, which starts from +0) and written
// once per pass.
template <class R>
__global__ __launch_bounds__(256) void accumulate_moments_kernel(const typename VecOf<R>::type* __restrict__ partial,
                                                                 typename VecOf<R>::type* __restrict__ acc, d4* __restrict__ q,
                                                                 R* __restrict__ out, const uint32_t* __restrict__ sizes,
                                                                 uint32_t shard_pixels, uint32_t chunks, uint32_t samples_done,
                                                                 uint32_t first) {
    typedef typename VecOf<R>::type r4;
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= shard_pixels) return;
    R x = 0, y = 0, z = 0;
    double qx = 0, qy = 0, qz = 0;
    if (!first) {
        const r4 a = acc[lp];
        const d4 m = q[lp];
        x = a.x, y = a.y, z = a.z;
        qx = m.x, qy = m.y, qz = m.z;
    }
    for (uint32_t k = 0; k < chunks; ++k) {
        const r4 p = partial[(size_t)k * shard_pixels + lp];
        const double n = (double)(sizes[k + 1] - sizes[k]);
        x = x + p.x;
        y = y + p.y;
        z = z + p.z;
        nz_fold<R>(qx, p.x, n);
        nz_fold<R>(qy, p.y, n);
        nz_fold<R>(qz, p.z, n);
    }
    acc[lp] = r4{x, y, z, R(0)};
    q[lp] = d4{qx, qy, qz, 0.0};
    if (out) {
        const R inv = R(1) / (R)samples_done;
        out[3 * (size_t)lp + 0] = x * inv;
        out[3 * (size_t)lp + 1] = y * inv;
        out[3 * (size_t)lp + 2] = z * inv;
    }
}

// ---- evaluation: one thread per pixel --------------------------------------------------------------------------------------
// Per pixel: var and rel2 (f32 = the f64 value rounded once; the f64 outputs exist for rayz_hip_noise_kat).  Summary, all
// deterministic: summary[0] += pixels with !(rel2 <= tau2) (integer atomic); summary[1] = max of rel2's bit pattern, sign bit
// cleared (integer atomic max: among non-negative doubles the patterns sort as the values do, and a NaN's sorts above +inf);
// block_sum[block] = Σ finite var of the block's pixels in a fixed order — lanes by a butterfly (offsets 32, 16, .., 1), then
// the four waves in wave order; the host adds the blocks in block order.  One wave-level reduction, then one block-level
// reduction through LDS, then at most two atomics per block.
template <class R>
__global__ __launch_bounds__(256) void noise_eval_kernel(const typename VecOf<R>::type* __restrict__ acc, const d4* __restrict__ q,
                                                         float* __restrict__ var_out, float* __restrict__ rel2_out,
                                                         double* __restrict__ var64_out, double* __restrict__ rel264_out,
                                                         unsigned long long* __restrict__ summary, double* __restrict__ block_sum,
                                                         uint32_t shard_pixels, uint32_t chunks_done, uint32_t samples_done,
                                                         double floor2, double tau2) {
    typedef typename VecOf<R>::type r4;
    __shared__ double s_sum[4];
    __shared__ unsigned long long s_max[4];
    __shared__ uint32_t s_cnt[4];
    const uint32_t lp = blockIdx.x * 256 + threadIdx.x;
    const bool live = lp < shard_pixels;
    double sum = 0.0;
    unsigned long long mx = 0;
    bool unconverged = false;
    if (live) { // (no early return: every lane takes part in the reductions below)
        const r4 a = acc[lp];
        const d4 m = q[lp];
        const NzEval e = nz_eval((double)a.x, (double)a.y, (double)a.z, m.x, m.y, m.z, (double)chunks_done, (double)samples_done, floor2);
        if (var_out) var_out[lp] = (float)e.var;
        if (rel2_out) rel2_out[lp] = (float)e.rel2;
        if (var64_out) var64_out[lp] = e.var;
        if (rel264_out) rel264_out[lp] = e.rel2;
        unconverged = !(e.rel2 <= tau2);
        mx = (unsigned long long)__double_as_longlong(e.rel2) & 0x7fffffffffffffffull;
        if (__builtin_isfinite(e.var)) sum = e.var;
    }
    const uint32_t cnt = (uint32_t)__popcll(__ballot(unconverged));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sum = sum + __shfl_xor(sum, off);
        const unsigned long long o = __shfl_xor(mx, off);
        mx = o > mx ? o : mx;
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_sum[wave] = sum, s_max[wave] = mx, s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        block_sum[blockIdx.x] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        const uint32_t c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        unsigned long long m = s_max[0];
        for (int w = 1; w < 4; ++w) m = s_max[w] > m ? s_max[w] : m;
        if (c) atomicAdd(&summary[0], (unsigned long long)c);
        if (m) atomicMax(&summary[1], m);
    }
}

// The same evaluation for an adaptive handle: every pixel with its own (K_i, N_i) — K_i = frozen_at[i], or
// chunks_done where that is 0, and N_i = starts[K_i].  A kernel of its own, its text repeated, so that noise_eval_kernel stays
// the kernel it was, instruction for instruction (as a shared body function it came out with two conversions reordered).
template <class R>
__global__ __launch_bounds__(256) void noise_eval_adaptive_kernel(const typename VecOf<R>::type* __restrict__ acc, const d4* __restrict__ q,
                                                                  float* __restrict__ var_out, float* __restrict__ rel2_out,
                                                                  double* __restrict__ var64_out, double* __restrict__ rel264_out,
                                                                  unsigned long long* __restrict__ summary, double* __restrict__ block_sum,
                                                                  uint32_t shard_pixels, uint32_t chunks_done, uint32_t samples_done,
                                                                  double floor2, double tau2, const uint32_t* __restrict__ frozen_at,
                                                                  const uint32_t* __restrict__ starts) {
    typedef typename VecOf<R>::type r4;
    __shared__ double s_sum[4];
    __shared__ unsigned long long s_max[4];
    __shared__ uint32_t s_cnt[4];
    const uint32_t lp = blockIdx.x * 256 + threadIdx.x;
    const bool live = lp < shard_pixels;
    double sum = 0.0;
    unsigned long long mx = 0;
    bool unconverged = false;
    if (live) { // (no early return: every lane takes part in the reductions below)
        const r4 a = acc[lp];
        const d4 m = q[lp];
        const uint32_t f = frozen_at[lp], K = f ? f : chunks_done, N = f ? starts[f] : samples_done;
        const NzEval e = nz_eval((double)a.x, (double)a.y, (double)a.z, m.x, m.y, m.z, (double)K, (double)N, floor2);
        if (var_out) var_out[lp] = (float)e.var;
        if (rel2_out) rel2_out[lp] = (float)e.rel2;
        if (var64_out) var64_out[lp] = e.var;
        if (rel264_out) rel264_out[lp] = e.rel2;
        unconverged = !(e.rel2 <= tau2);
        mx = (unsigned long long)__double_as_longlong(e.rel2) & 0x7fffffffffffffffull;
        if (__builtin_isfinite(e.var)) sum = e.var;
    }
    const uint32_t cnt = (uint32_t)__popcll(__ballot(unconverged));
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        sum = sum + __shfl_xor(sum, off);
        const unsigned long long o = __shfl_xor(mx, off);
        mx = o > mx ? o : mx;
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_sum[wave] = sum, s_max[wave] = mx, s_cnt[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        block_sum[blockIdx.x] = ((s_sum[0] + s_sum[1]) + s_sum[2]) + s_sum[3];
        const uint32_t c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        unsigned long long m = s_max[0];
        for (int w = 1; w < 4; ++w) m = s_max[w] > m ? s_max[w] : m;
        if (c) atomicAdd(&summary[0], (unsigned long long)c);
        if (m) atomicMax(&summary[1], m);
    }
}

// ---- the per-channel variance (rayz_hip_progressive_noise_rgb): one thread per pixel ------------------------------------------
// var_ch = D_ch / ((K - 1) · N) with §4.12's D_ch, its clamp included: the terms nz_eval sums, kept apart, for a consumer that
// filters each channel on its own scale (the guided denoiser, §4.13).  f64, rounded once to f32; K < 2: +inf.  Three floats per
// pixel, packed as frames are.
template <class R>
__global__ __launch_bounds__(256) void noise_rgb_kernel(const typename VecOf<R>::type* __restrict__ acc, const d4* __restrict__ q,
                                                        float* __restrict__ var_rgb, uint32_t shard_pixels, uint32_t chunks_done,
                                                        uint32_t samples_done) {
    typedef typename VecOf<R>::type r4;
    const uint32_t lp = blockIdx.x * 256 + threadIdx.x;
    if (lp >= shard_pixels) return;
    const double K = (double)chunks_done, N = (double)samples_done;
    double vr = __builtin_inf(), vg = vr, vb = vr;
    if (!(K < 2.0)) {
        const r4 a = acc[lp];
        const d4 m = q[lp];
        const double Mr = (double)a.x, Mg = (double)a.y, Mb = (double)a.z;
        double Dr = m.x - (Mr * Mr) / N, Dg = m.y - (Mg * Mg) / N, Db = m.z - (Mb * Mb) / N;
        Dr = Dr < 0.0 ? 0.0 : Dr; // (a NaN stays a NaN)
        Dg = Dg < 0.0 ? 0.0 : Dg;
        Db = Db < 0.0 ? 0.0 : Db;
        const double d = (K - 1.0) * N;
        vr = Dr / d, vg = Dg / d, vb = Db / d;
    }
    var_rgb[3 * (size_t)lp + 0] = (float)vr;
    var_rgb[3 * (size_t)lp + 1] = (float)vg;
    var_rgb[3 * (size_t)lp + 2] = (float)vb;
}

// .. and for an adaptive handle, (K_i, N_i) per pixel as noise_eval_adaptive_kernel takes them.
template <class R>
__global__ __launch_bounds__(256) void noise_rgb_adaptive_kernel(const typename VecOf<R>::type* __restrict__ acc, const d4* __restrict__ q,
                                                                 float* __restrict__ var_rgb, uint32_t shard_pixels, uint32_t chunks_done,
                                                                 uint32_t samples_done, const uint32_t* __restrict__ frozen_at,
                                                                 const uint32_t* __restrict__ starts) {
    typedef typename VecOf<R>::type r4;
    const uint32_t lp = blockIdx.x * 256 + threadIdx.x;
    if (lp >= shard_pixels) return;
    const uint32_t f = frozen_at[lp];
    const double K = (double)(f ? f : chunks_done), N = (double)(f ? starts[f] : samples_done);
    double vr = __builtin_inf(), vg = vr, vb = vr;
    if (!(K < 2.0)) {
        const r4 a = acc[lp];
        const d4 m = q[lp];
        const double Mr = (double)a.x, Mg = (double)a.y, Mb = (double)a.z;
        double Dr = m.x - (Mr * Mr) / N, Dg = m.y - (Mg * Mg) / N, Db = m.z - (Mb * Mb) / N;
        Dr = Dr < 0.0 ? 0.0 : Dr; // (a NaN stays a NaN)
        Dg = Dg < 0.0 ? 0.0 : Dg;
        Db = Db < 0.0 ? 0.0 : Db;
        const double d = (K - 1.0) * N;
        vr = Dr / d, vg = Dg / d, vb = Db / d;
    }
    var_rgb[3 * (size_t)lp + 0] = (float)vr;
    var_rgb[3 * (size_t)lp + 1] = (float)vg;
    var_rgb[3 * (size_t)lp + 2] = (float)vb;
}

inline uint32_t noise_blocks(uint64_t pixels) { return (uint32_t)((pixels + 255) / 256); }

} // namespace rayz_dev
