// temporal_cubic_kernel.hpp — the device code of temporal accumulation's cubic resampling mode (include/rayz_hip.h:
// rayz_hip_temporal_set_resampling; the host side: temporal.hpp, temporal_moments.hpp).
//
// Two kernels, the moving forms of the plain and of the moments step of a handle in RAYZ_TEMPORAL_RESAMPLE_CUBIC (a static step
// resamples nothing and launches the existing static kernels).  The moments one is tm_step (temporal_moments_kernel.hpp) with its
// CUBIC flag, below; the plain one is ta_mode_step with its CUBIC flag (temporal_modes_kernel.hpp), because temporal_step_kernel's
// body is the __global__ function itself and its code is held instruction-identical.
//
// Both run ta_gather first, unchanged, and have it keep its four taps: §4.15 steps 1-3 are stated once, and the variance, W2 and the
// length are the bilinear values in both modes.  Then tc_resample, for a pixel whose four inner taps were all accepted and whose 4x4 window lies
// inside the frame, the twelve outer taps in four rounds, one row of the window each (rows −1 and 2 bring four taps, rows 0 and 1
// two): a round loads its taps' guide pairs and records together and unconditionally, so a wave waits for memory once per round;
// the first refused tap ends the pixel's cubic path, and the pixel keeps the bilinear result.  Holding all sixteen taps at once
// would be 16 x (2 + R) x 4 registers; a round holds at most four.  The inner taps' records are ta_gather's own loads: they join
// the sums in contract order (j outer, i inner) and give the clamp its range.  No LDS for the taps: their position is
// data-dependent, as in the plain kernel.
#pragma once

#include "temporal_moments_kernel.hpp"

namespace rayz_dev {

// §4.26's four weights of a fraction f: Catmull-Rom (a = −0.5) in Horner form.  f = 0 gives (0, 1, 0, 0), f = 1 (0, 0, 1, 0), exactly.
__device__ __forceinline__ void tc_weights(float f, float (&w)[4]) {
    const float f2 = f * f;
    w[0] = f * __builtin_fmaf(f, __builtin_fmaf(-0.5f, f, 1.0f), -0.5f);
    w[1] = __builtin_fmaf(f2, __builtin_fmaf(1.5f, f, -2.5f), 1.0f);
    w[2] = f * __builtin_fmaf(f, __builtin_fmaf(-1.5f, f, 2.0f), 0.5f);
    w[3] = f2 * __builtin_fmaf(0.5f, f, -0.5f);
}

// hc clamped to the range of the four inner taps' values, by comparisons in tap order.
__device__ __forceinline__ float tc_clamp(float hc, float t0, float t1, float t2, float t3) {
    float lo = t0, hi = t0;
    lo = t1 < lo ? t1 : lo, hi = t1 > hi ? t1 : hi;
    lo = t2 < lo ? t2 : lo, hi = t2 > hi ? t2 : hi;
    lo = t3 < lo ? t3 : lo, hi = t3 > hi ? t3 : hi;
    return hc < lo ? lo : (hc > hi ? hi : hc);
}

// §4.26 for one pixel that found bilinear history (ta_gather's acc.found(), so the taps in k are set): true where the cubic path is
// taken, and then h[r][ch] is the clamped cubic value of channel ch of record r < NC (the plain step: 1, the colour — its variance
// stays bilinear; the moments step: 2, the colour and m2).  rec: ta_gather's.
template <int NC>
__device__ __forceinline__ bool tc_resample(const TemporalArgs& a, const dn4* const* rec, const TaTaps<2>& k, int32_t id, float nx,
                                            float ny, float nz, float Px, float Py, float Pz, float (&h)[NC][3]) {
    static_assert(NC == 1 || NC == 2, "the colour, or the colour and the second record");
    // All sixteen taps inside the frame — so every address below is a pixel's — and the inner four accepted.
    bool go = k.ok[0] && k.ok[1] && k.ok[2] && k.ok[3] && k.ix >= 1 && k.ix + 2 < (int)a.width && k.iy >= 1 && k.iy + 2 < (int)a.height;
    float wx[4], wy[4];
    tc_weights(k.fx, wx);
    tc_weights(k.fy, wy);
    float W = 0.0f, C[NC][3] = {};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (go) {
            const bool whole = j == 0 || j == 3; // rows −1 and 2: four new taps; rows 0 and 1: the two beside the inner pair
            const size_t row = (size_t)(k.iy + j - 1) * a.width + (size_t)(k.ix - 1);
            dn4 g[4], pp[4], c[4][NC];
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (whole || i == 0 || i == 3) {
                    g[i] = a.prev.g[row + i], pp[i] = a.prev.p[row + i];
#pragma unroll
                    for (int r = 0; r < NC; ++r) c[i][r] = rec[r][row + i];
                }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (whole || i == 0 || i == 3) go = go && ta_accepts(a, g[i], pp[i], id, nx, ny, nz, Px, Py, Pz, k.lim);
            if (go) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float b = wx[i] * wy[j];
                    W = W + b;
#pragma unroll
                    for (int r = 0; r < NC; ++r) {
                        const dn4 v = (whole || i == 0 || i == 3) ? c[i][r] : k.tap[2 * (j - 1) + (i - 1)][r];
                        C[r][0] = __builtin_fmaf(b, v.x, C[r][0]);
                        C[r][1] = __builtin_fmaf(b, v.y, C[r][1]);
                        C[r][2] = __builtin_fmaf(b, v.z, C[r][2]);
                    }
                }
            }
        }
    }
    if (go) {
#pragma unroll
        for (int r = 0; r < NC; ++r)
#pragma unroll
            for (int ch = 0; ch < 3; ++ch)
                h[r][ch] = tc_clamp(C[r][ch] / W, k.tap[0][r][ch], k.tap[1][r][ch], k.tap[2][r][ch], k.tap[3][r][ch]);
    }
    return go;
}

} // namespace rayz_dev

// The kernels live in a namespace of their own: the kernels of rayz_dev are a recorded set (tests/test_slab_cells_isa.py).
namespace rayz_dev_cubic {
using namespace rayz_dev;

struct TemporalCubicMomentsArgs {
    TemporalMomentsArgs m;
    uint8_t* taken; // or NULL: one byte per pixel, 1 where the colour history came from the sixteen taps
};

__global__ __launch_bounds__(256) void temporal_cubic_moments_step_kernel(const TemporalCubicMomentsArgs a) {
    __shared__ dn4 s_col[kTmLdsH * kTmLdsW], s_nrm[kTmLdsH * kTmLdsW];
    TcPixel tc;
    tc.taken = a.taken;
    tm_step<false, false>(a.m, s_col, s_nrm, &tc);
}

} // namespace rayz_dev_cubic
