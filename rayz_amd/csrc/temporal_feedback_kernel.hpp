// temporal_feedback_kernel.hpp — the device code of temporal accumulation's feedback mode (include/rayz_hip.h:
// rayz_hip_temporal_track_feedback, rayz_hip_temporal_feedback; the handle and the validation: temporal_moments.hpp).
//
// SVGF writes the output of its first à-trous level back as the colour history, so the next frame blends into a colour that has
// been smoothed once — while the variance still has to come from RAW moments.  Two kernels:
//
// The STEP is the moments step's body (temporal_moments_kernel.hpp: tm_step) with FEEDBACK = true: the history's v record, which a
// moments step writes and never reads, holds {m1.r, m1.g, m1.b, 0} instead — the raw first moment, what the colour would be had no
// feedback ever been given.  Every accepted tap reads it too (one more 16-byte record per tap, in the second round of loads), it is
// blended exactly as the colour is, and §4.16's step 3 takes it where it takes the colour.  LDS, the vote and the barriers are the
// moments step's; the launch is temporal_kernel.hpp's temporal_launch_step, as every step's.
//
// The WRITE replaces {c.r, c.g, c.b} of the history side the last step wrote with the caller's pixel and leaves the length in
// c.w: a streaming kernel on the 32x8 tiles, 12 bytes read and one 16-byte record read and written per pixel, no LDS.  A pixel with
// a channel that is not finite keeps its colour: a NaN in the history would otherwise stay until a disocclusion.
#pragma once

#include "temporal_moments_kernel.hpp"

namespace rayz_dev {

template <bool STATIC> __global__ __launch_bounds__(256) void temporal_feedback_step_kernel(const TemporalMomentsArgs m) {
    __shared__ dn4 s_col[kTmLdsH * kTmLdsW], s_nrm[kTmLdsH * kTmLdsW];
    tm_step<STATIC, true>(m, s_col, s_nrm);
}

__device__ __forceinline__ bool tf_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(256) void temporal_feedback_write_kernel(dn4* __restrict__ c, const float* __restrict__ rgb, uint32_t width,
                                                                      uint32_t height) {
    const int x = (int)(blockIdx.x * kDnTileW + threadIdx.x % kDnTileW);
    const int y = (int)(blockIdx.y * kDnTileH + threadIdx.x / kDnTileW);
    if (x >= (int)width || y >= (int)height) return;
    const size_t p = (size_t)y * width + (size_t)x;
    const float r = rgb[3 * p], g = rgb[3 * p + 1], b = rgb[3 * p + 2];
    const dn4 was = c[p];
    if (tf_finite(r) && tf_finite(g) && tf_finite(b)) c[p] = dn4{r, g, b, was.w};
}

// ---- host side: the write's launch (the steps': temporal_kernel.hpp; temporal_moments.hpp owns the validation) -------------------
inline void temporal_feedback_launch_write(hipStream_t st, dn4* c, const float* rgb, uint32_t width, uint32_t height) {
    hipLaunchKernelGGL(temporal_feedback_write_kernel, denoise_grid(width, height), dim3(256), 0, st, c, rgb, width, height);
}

} // namespace rayz_dev
