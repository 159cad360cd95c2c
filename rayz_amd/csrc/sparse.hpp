// sparse.hpp — sparse renders' device code (include/rayz_hip.h: rayz_hip_scene_render_pixels[_f64]).
//
// A sparse render traces a caller's list of local pixels through the adaptive-pass kernels (§4.14: chunk k of entry j leaves its
// sum at the compact index k · n + j) and resolves each entry into the slot the caller names.  Nothing here is new arithmetic:
// the colour is resolve_kernel's (the chunk sums added in chunk order from +0, times 1 / spp), the variance noise_rgb_kernel's
// (§4.12) on the Q that nz_fold builds from the same chunk sums — what a tracked progressive handle holds once every chunk is
// folded.  tests/sparse_ref.py restates the resolve in numpy.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "device_types.hpp"
#include "noise.hpp"

namespace rayz_dev {

// *bad += the entries with pixels[j] >= shard_pixels or (with `dest`) dest[j] >= dest_pixels: one ballot per wave, one atomic per
// wave that found any.  The host launches nothing that indexes with an entry unless the count stays 0.
__global__ __launch_bounds__(256) void sparse_check_kernel(const uint32_t* __restrict__ pixels, const uint32_t* __restrict__ dest, uint32_t n,
                                                           uint32_t shard_pixels, uint32_t dest_pixels, uint32_t* __restrict__ bad) {
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    bool wrong = false;
    if (j < n) wrong = pixels[j] >= shard_pixels || (dest && dest[j] >= dest_pixels); // (no early return: every lane votes)
    const uint32_t cnt = (uint32_t)__popcll(__ballot(wrong));
    if ((threadIdx.x & 63) == 0 && cnt) atomicAdd(bad, cnt);
}

// One thread per entry j: its `chunks` compact chunk sums partial[k · n + j] in chunk order from +0, the pixel into slot dest[j]
// (j without `dest`) of `out`, and with VAR the per-channel variance of its mean into the same slot of `var_out`.  `sizes` is
// the whole schedule (chunk k holds sizes[k + 1] - sizes[k] samples), chunks_total its length and spp its end: K and N of the
// estimate.  chunks = 0 with chunks_total > 0 is the render that traces nothing (max_bounces = 0): sums and Q stay +0, as a
// tracked handle's do.
template <class R, bool VAR>
__global__ __launch_bounds__(256) void sparse_resolve_kernel(const typename VecOf<R>::type* __restrict__ partial,
                                                             const uint32_t* __restrict__ dest, uint32_t n, R* __restrict__ out,
                                                             float* __restrict__ var_out, const uint32_t* __restrict__ sizes,
                                                             uint32_t chunks, uint32_t chunks_total, uint32_t spp) {
    typedef typename VecOf<R>::type r4;
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    R x = 0, y = 0, z = 0;
    double qx = 0, qy = 0, qz = 0;
    for (uint32_t k = 0; k < chunks; ++k) {
        const r4 p = partial[(size_t)k * n + j];
        x = x + p.x;
        y = y + p.y;
        z = z + p.z;
        if (VAR) {
            const double m = (double)(sizes[k + 1] - sizes[k]);
            nz_fold<R>(qx, p.x, m);
            nz_fold<R>(qy, p.y, m);
            nz_fold<R>(qz, p.z, m);
        }
    }
    const size_t slot = dest ? dest[j] : j;
    const R inv = R(1) / (R)spp;
    out[3 * slot + 0] = x * inv;
    out[3 * slot + 1] = y * inv;
    out[3 * slot + 2] = z * inv;
    if (VAR) {
        const double K = (double)chunks_total, N = (double)spp;
        double vr = __builtin_inf(), vg = vr, vb = vr;
        if (!(K < 2.0)) {
            const double Mr = (double)x, Mg = (double)y, Mb = (double)z;
            double Dr = qx - (Mr * Mr) / N, Dg = qy - (Mg * Mg) / N, Db = qz - (Mb * Mb) / N;
            Dr = Dr < 0.0 ? 0.0 : Dr; // (a NaN stays a NaN)
            Dg = Dg < 0.0 ? 0.0 : Dg;
            Db = Db < 0.0 ? 0.0 : Db;
            const double d = (K - 1.0) * N;
            vr = Dr / d, vg = Dg / d, vb = Db / d;
        }
        var_out[3 * slot + 0] = (float)vr;
        var_out[3 * slot + 1] = (float)vg;
        var_out[3 * slot + 2] = (float)vb;
    }
}

} // namespace rayz_dev
