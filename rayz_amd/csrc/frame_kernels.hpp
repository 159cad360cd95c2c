// frame_kernels.hpp — from chunk sums to a frame: resolve_kernel (a pixel's chunk sums in chunk order, src/renderer.zig:94-95),
// accumulate_kernel (the same sum cut at the progressive passes' boundaries) and tonemap_kernel (writePPM's per-pixel transform).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.hpp"

namespace rayz_dev {

// ---- pixel = (Σ_chunks partial) · (1/spp), chunk order: src/renderer.zig:94-95 ---------------------
template <class R>
__global__ __launch_bounds__(256) void resolve_kernel(const typename VecOf<R>::type* __restrict__ partial,
                                                      R* __restrict__ out, uint32_t shard_pixels,
                                                      uint32_t chunks_per_px, uint32_t spp) {
    typedef typename VecOf<R>::type r4;
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= shard_pixels) return;
    R x = 0, y = 0, z = 0;
    for (uint32_t k = 0; k < chunks_per_px; ++k) {
        const r4 p = partial[(size_t)k * shard_pixels + lp];
        x = x + p.x;
        y = y + p.y;
        z = z + p.z;
    }
    const R inv = R(1) / (R)spp;
    out[3 * (size_t)lp + 0] = x * inv;
    out[3 * (size_t)lp + 1] = y * inv;
    out[3 * (size_t)lp + 2] = z * inv;
}

// ---- progressive passes: acc = acc + partial[k] for the pass's chunks in chunk order; preview = acc · (1/samples_done) ------
// resolve_kernel's loop cut at the passes' boundaries: the same additions in the same order, the running sum kept in `acc`
// between passes (stored in R, so nothing is rounded that resolve_kernel keeps in a register).  After the last pass acc holds
// resolve_kernel's x bit for bit and the preview (samples_done = spp) is its pixel.  `first`: the pass that starts at chunk 0
// begins from +0, as resolve_kernel does, without reading acc.  A streaming kernel: one 16-byte (f32) load per chunk and pixel.
template <class R>
__global__ __launch_bounds__(256) void accumulate_kernel(const typename VecOf<R>::type* __restrict__ partial,
                                                         typename VecOf<R>::type* __restrict__ acc, R* __restrict__ out,
                                                         uint32_t shard_pixels, uint32_t chunks, uint32_t samples_done,
                                                         uint32_t first) {
    typedef typename VecOf<R>::type r4;
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= shard_pixels) return;
    R x = 0, y = 0, z = 0;
    if (!first) {
        const r4 a = acc[lp];
        x = a.x, y = a.y, z = a.z;
    }
    for (uint32_t k = 0; k < chunks; ++k) {
        const r4 p = partial[(size_t)k * shard_pixels + lp];
        x = x + p.x;
        y = y + p.y;
        z = z + p.z;
    }
    acc[lp] = r4{x, y, z, R(0)};
    if (out) {
        const R inv = R(1) / (R)samples_done;
        out[3 * (size_t)lp + 0] = x * inv;
        out[3 * (size_t)lp + 1] = y * inv;
        out[3 * (size_t)lp + 2] = z * inv;
    }
}

// ---- `writePPM`'s per-pixel transform, src/image.zig:35-38 + src/vec.zig:79-93 -------------------
__global__ __launch_bounds__(256) void tonemap_kernel(const float* __restrict__ rgb, uint8_t* __restrict__ out,
                                                      size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // in f64, as writePPM computes it on the widened pixel: bit-identical to the host writer
    const double v = (double)rgb[i];
    double s = v > 0.0 ? __builtin_sqrt(v) : 0.0;
    s = s > 0.0 ? s : 0.0; // utils.max(x, low)
    s = s < 1.0 ? s : 1.0; // utils.min(.., high)
    out[i] = (uint8_t)(s * 255.0);
}

} // namespace rayz_dev
