// footprint.hpp — the footprint albedo's device code (include/rayz_hip.h: rayz_hip_upscaler_footprint_albedo; the
// host side: upscaler.hpp).
//
// A pixel of a frame traced at 1/f of the resolution (render.lowres_camera) is the mean over its f x f block of full pixels, but
// the albedo of its G-buffer is ONE point sample at the block's centre: where the texture is finer than a low-resolution pixel,
// demodulating the block mean by that sample is off by the texture's contrast.  This pass gives every low-resolution pixel the
// mean of the full-size albedos of its block that lie on ITS surface — the same hittable index, an integer decision —, which is
// what the upscaler's pack pass should divide by.  The raw albedo is averaged; the clamp to 2^-8 stays in the pack pass.
//
// The arithmetic is a contract (§4.24, the rules of §4.11): plain f32 adds in the order dy outer, dx inner, one correctly rounded
// divide, integer compares, selections; no FMA — restated bit for bit by tests/footprint_mirror.cpp.
//
// One thread per LOW-resolution pixel, 32x8 tiles, lanes along x: for each dy a wave reads one contiguous span of 64·f full pixels
// of the index (4 bytes each) and of the albedo (12 bytes each), a lane taking f neighbouring pixels of it; the f x f loop is
// unrolled, every load of a block is issued whether or not its pixel matches (the block lies inside the full frame whenever its
// low-resolution pixel lies inside its own), and the sums are built by selection.  No LDS.
//
// The kernel lives in a namespace of its own: rayz_dev holds exactly the kernels it held.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace rayz_dev_footprint {

constexpr int kTileW = 32, kTileH = 8; // low-resolution pixels of a workgroup: 256 threads, a wave covers two tile rows

// F: the factor.  COUNT: the number of matching pixels is written too.  (w, h): the low-resolution frame; the full one is F times it.
template <int F, bool COUNT>
__global__ __launch_bounds__(256) void footprint_albedo_kernel(const int32_t* __restrict__ index_lo, const float* __restrict__ albedo_lo,
                                                                const int32_t* __restrict__ index_hi, const float* __restrict__ albedo_hi,
                                                                float* __restrict__ out, uint8_t* __restrict__ count, const uint32_t w,
                                                                const uint32_t h) {
    const uint32_t i = blockIdx.x * kTileW + threadIdx.x % kTileW;
    const uint32_t j = blockIdx.y * kTileH + threadIdx.x / kTileW;
    if (i >= w || j >= h) return;
    const size_t q = (size_t)j * w + i;
    const int32_t id = index_lo[q];
    const size_t full_w = (size_t)F * w;
    uint32_t n = 0;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f;
#pragma unroll
    for (int dy = 0; dy < F; ++dy) {
        const size_t row = ((size_t)F * j + dy) * full_w + (size_t)F * i;
#pragma unroll
        for (int dx = 0; dx < F; ++dx) {
            const size_t p = row + dx;
            const bool same = index_hi[p] == id;
            const float ar = albedo_hi[3 * p], ag = albedo_hi[3 * p + 1], ab = albedo_hi[3 * p + 2];
            n += same ? 1u : 0u;
            const bool add = same && id >= 0;
            sr = add ? sr + ar : sr;
            sg = add ? sg + ag : sg;
            sb = add ? sb + ab : sb;
        }
    }
    float r, g, b;
    if (id < 0) { // background: m = 1 whatever the albedo arrays hold
        r = g = b = 1.0f;
    } else if (n == 0) { // no centre of the block lies on q's surface: the point sample, its bits
        r = albedo_lo[3 * q], g = albedo_lo[3 * q + 1], b = albedo_lo[3 * q + 2];
    } else {
        const float fn = (float)n;
        r = sr / fn, g = sg / fn, b = sb / fn;
    }
    out[3 * q] = r;
    out[3 * q + 1] = g;
    out[3 * q + 2] = b;
    if (COUNT) count[q] = (uint8_t)n;
}

// ---- host side: the launch (upscaler.hpp owns the handle, the validation and the stream) ---------------------------------------
template <int F>
inline void footprint_launch_f(hipStream_t st, const int32_t* index_lo, const float* albedo_lo, const int32_t* index_hi, const float* albedo_hi,
                               float* out, uint8_t* count, uint32_t w, uint32_t h) {
    const dim3 grid((w + kTileW - 1) / kTileW, (h + kTileH - 1) / kTileH);
    if (count) hipLaunchKernelGGL((footprint_albedo_kernel<F, true>), grid, dim3(256), 0, st, index_lo, albedo_lo, index_hi, albedo_hi, out, count, w, h);
    else hipLaunchKernelGGL((footprint_albedo_kernel<F, false>), grid, dim3(256), 0, st, index_lo, albedo_lo, index_hi, albedo_hi, out, count, w, h);
}

// `factor` is 2, 3 or 4 (the handle's: checked at its creation).
inline void footprint_launch(hipStream_t st, uint32_t factor, const int32_t* index_lo, const float* albedo_lo, const int32_t* index_hi,
                             const float* albedo_hi, float* out, uint8_t* count, uint32_t w, uint32_t h) {
    if (factor == 2) footprint_launch_f<2>(st, index_lo, albedo_lo, index_hi, albedo_hi, out, count, w, h);
    else if (factor == 3) footprint_launch_f<3>(st, index_lo, albedo_lo, index_hi, albedo_hi, out, count, w, h);
    else footprint_launch_f<4>(st, index_lo, albedo_lo, index_hi, albedo_hi, out, count, w, h);
}

} // namespace rayz_dev_footprint
