// temporal_counts_kernel.hpp — the device code of temporal accumulation's counts step (include/rayz_hip.h:
// rayz_hip_temporal_step_counts, rayz_hip_temporal_step_moments_counts; the host side: temporal.hpp, temporal_moments.hpp; the steps
// it is made from: temporal_kernel.hpp, temporal_moments_kernel.hpp).
//
// The plain and the moments step with ONE difference: the samples the current frame adds are a number per pixel, read from an
// array of height·width uint32, and may be 0 — a lattice frame (§4.21) samples one pixel in f², an adaptive frame (§4.14) as many
// as each pixel still needs.  Three rules follow (§4.23): a history record of length 0 holds no samples and is refused like a
// different surface (ta_gather's LIVE flag); a pixel that got no sample and finds history keeps the gathered history, by
// selection, so that whatever its input holds — NaN included — reaches nothing; and the moments step's 7x7 neighbourhood counts
// only positions that were sampled.  Everything else is the scalar steps' arithmetic, through the same functions: with
// every count equal to one spp >= 1 the four kernels below return what temporal_step_kernel and temporal_moments_step_kernel return,
// bit for bit.  Per pixel they read 4 more bytes than their twins; the moments pair stages the count in the free lane of the
// staged normal record, so the LDS and the barriers are the twin's.
//
// The kernels live in a namespace of their own: rayz_dev holds exactly the kernels it held.
#pragma once

#include "temporal_moments_kernel.hpp"

namespace rayz_dev_counts {
using namespace rayz_dev;

struct TemporalCountsArgs {
    TemporalArgs t;         // the plain step's arguments; t.spp is not read
    const uint32_t* counts; // per pixel: the samples the current frame adds (never an output: a pixel reads its neighbours' too)
};

struct TemporalMomentsCountsArgs {
    TemporalMomentsArgs m; // the moments step's arguments; m.t.spp is not read
    const uint32_t* counts;
};

// §4.23 on §4.15: the plain step's body with n = f32(count) for spp, the LIVE gather and the selection for n = 0.
template <bool STATIC> __global__ __launch_bounds__(256) void temporal_counts_kernel(const TemporalCountsArgs ca) {
    const TemporalArgs& a = ca.t;
    const int x = (int)(blockIdx.x * kDnTileW + threadIdx.x % kDnTileW);
    const int y = (int)(blockIdx.y * kDnTileH + threadIdx.x / kDnTileW);
    if (x >= (int)a.width || y >= (int)a.height) return;
    const size_t p = (size_t)y * a.width + (size_t)x;
    const float cr = a.rgb[3 * p], cg = a.rgb[3 * p + 1], cb = a.rgb[3 * p + 2];
    const float sr = dn_clamp_var(a.var[3 * p]), sg = dn_clamp_var(a.var[3 * p + 1]), sb = dn_clamp_var(a.var[3 * p + 2]);
    const int32_t id = a.index[p];
    const float nx = a.normal[3 * p], ny = a.normal[3 * p + 1], nz = a.normal[3 * p + 2];
    const float Px = a.point[3 * p], Py = a.point[3 * p + 1], Pz = a.point[3 * p + 2];
    const float n = (float)ca.counts[p];
    float or_ = cr, og = cg, ob = cb, vr = sr, vg = sg, vb = sb, No = n; // no history: the input, by selection
    if (id >= 0 && a.has_history) {
        const dn4* const rec[2] = {a.prev.c, a.prev.v};
        const TaAcc<2> acc = ta_gather<STATIC, 2, true>(a, rec, p, id, nx, ny, nz, Px, Py, Pz);
        if (acc.found()) {
            const TaBlend h = ta_blend_head(acc, a, n);
            No = h.N; // (n = 0: hN + 0, capped)
            if (n > 0.0f) {
                const float a2 = h.al * h.al, k2 = h.k * h.k;
                or_ = ta_blend(h.al, cr, acc.mean(0, 0));
                og = ta_blend(h.al, cg, acc.mean(0, 1));
                ob = ta_blend(h.al, cb, acc.mean(0, 2));
                vr = __builtin_fmaf(a2, sr, k2 * acc.mean(1, 0));
                vg = __builtin_fmaf(a2, sg, k2 * acc.mean(1, 1));
                vb = __builtin_fmaf(a2, sb, k2 * acc.mean(1, 2));
            } else { // no sample: the gathered history, by selection — the input is loaded and never used
                or_ = acc.mean(0, 0), og = acc.mean(0, 1), ob = acc.mean(0, 2);
                vr = acc.mean(1, 0), vg = acc.mean(1, 1), vb = acc.mean(1, 2);
            }
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

// §4.23 on §4.16: tm_step's body (temporal_moments_kernel.hpp, without its feedback mode) with n = f32(count) for spp, the LIVE
// gather, the selection for n = 0 and the neighbourhood over sampled positions.  A second body and not a flag of tm_step: the flag
// moved the instructions of the moments and feedback kernels.  The barriers are tm_step's — the vote and the barrier behind the
// staging are reached by all 256 threads, a thread outside the frame skips only the per-pixel work and the stores — and so is the
// LDS: two arrays of 38 x 14 records and the vote's; the count rides in the .w of the staged normal record.
template <bool STATIC> __global__ __launch_bounds__(256) void temporal_counts_moments_kernel(const TemporalMomentsCountsArgs ca) {
    __shared__ dn4 s_col[kTmLdsH * kTmLdsW], s_nrm[kTmLdsH * kTmLdsW];
    const TemporalMomentsArgs& m = ca.m;
    const TemporalArgs& a = m.t;
    const int tx = (int)(threadIdx.x % kDnTileW), ty = (int)(threadIdx.x / kDnTileW);
    const int x = (int)(blockIdx.x * kDnTileW) + tx, y = (int)(blockIdx.y * kDnTileH) + ty;
    const bool inside = x < (int)a.width && y < (int)a.height; // NO early return: every thread reaches the vote and the barrier
    const size_t p = inside ? (size_t)y * a.width + (size_t)x : 0;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, Px = 0.0f, Py = 0.0f, Pz = 0.0f;
    float or_ = 0.0f, og = 0.0f, ob = 0.0f, No = 0.0f, qr = 0.0f, qg = 0.0f, qb = 0.0f, W2 = 1.0f, vr = 0.0f, vg = 0.0f, vb = 0.0f;
    int32_t id = -1;
    bool spatial = false;
    if (inside) {
        const float cr = a.rgb[3 * p], cg = a.rgb[3 * p + 1], cb = a.rgb[3 * p + 2];
        const float n = (float)ca.counts[p];
        id = a.index[p];
        nx = a.normal[3 * p], ny = a.normal[3 * p + 1], nz = a.normal[3 * p + 2];
        Px = a.point[3 * p], Py = a.point[3 * p + 1], Pz = a.point[3 * p + 2];
        or_ = cr, og = cg, ob = cb, No = n;                  // no history: the input, by selection ..
        qr = cr * cr, qg = cg * cg, qb = cb * cb, W2 = 1.0f; // .. its square, and the weight of one frame
        if (id >= 0 && a.has_history) {
            const dn4* const rec[2] = {a.prev.c, m.prev_m};
            const TaAcc<2> acc = ta_gather<STATIC, 2, true>(a, rec, p, id, nx, ny, nz, Px, Py, Pz);
            if (acc.found()) {
                const TaBlend h = ta_blend_head(acc, a, n);
                No = h.N; // (n = 0: hN + 0, capped)
                if (n > 0.0f) {
                    or_ = ta_blend(h.al, cr, acc.mean(0, 0));
                    og = ta_blend(h.al, cg, acc.mean(0, 1));
                    ob = ta_blend(h.al, cb, acc.mean(0, 2));
                    qr = ta_blend(h.al, cr * cr, acc.mean(1, 0));
                    qg = ta_blend(h.al, cg * cg, acc.mean(1, 1));
                    qb = ta_blend(h.al, cb * cb, acc.mean(1, 2));
                    W2 = __builtin_fmaf(h.k * h.k, acc.mean(1, 3), h.al * h.al);
                } else { // no sample: the gathered means, by selection (al = 0, k = 1) — the input is loaded and never used
                    or_ = acc.mean(0, 0), og = acc.mean(0, 1), ob = acc.mean(0, 2);
                    qr = acc.mean(1, 0), qg = acc.mean(1, 1), qb = acc.mean(1, 2), W2 = acc.mean(1, 3);
                }
            }
        }
        spatial = id >= 0 && W2 > m.wm;
        if (id >= 0 && !spatial) vr = tm_temporal_var(qr, or_, W2), vg = tm_temporal_var(qg, og, W2), vb = tm_temporal_var(qb, ob, W2);
    }
    // The vote: reached by every thread of the workgroup; its result is the same in all of them.
    if (__syncthreads_or(spatial ? 1 : 0)) {
        const int bx = (int)(blockIdx.x * kDnTileW) - kTmHalo, by = (int)(blockIdx.y * kDnTileH) - kTmHalo;
        for (int t = (int)threadIdx.x; t < kTmLdsW * kTmLdsH; t += 256) { // (t < 532: inside both arrays)
            const int gx = bx + t % kTmLdsW, gy = by + t / kTmLdsW;
            dn4 vc{0.0f, 0.0f, 0.0f, __int_as_float(kTmOutside)}, vn{0.0f, 0.0f, 0.0f, 0.0f};
            if (gx >= 0 && gx < (int)a.width && gy >= 0 && gy < (int)a.height) { // (so q < width·height: inside counts too)
                const size_t q = (size_t)gy * a.width + (size_t)gx;
                vc = dn4{a.rgb[3 * q], a.rgb[3 * q + 1], a.rgb[3 * q + 2], __int_as_float(a.index[q])};
                vn = dn4{a.normal[3 * q], a.normal[3 * q + 1], a.normal[3 * q + 2], (float)ca.counts[q]};
            }
            s_col[t] = vc, s_nrm[t] = vn;
        }
        __syncthreads(); // all 256 threads are here: the branch is the workgroup's, not a thread's
        if (spatial) {
            float S0 = 0.0f, S1r = 0.0f, S1g = 0.0f, S1b = 0.0f, S2r = 0.0f, S2g = 0.0f, S2b = 0.0f;
            const int centre = (ty + kTmHalo) * kTmLdsW + tx + kTmHalo; // taps: centre + j·38 + i stays within [0, 532)
            for (int j = -kTmHalo; j <= kTmHalo; ++j)
#pragma unroll
                for (int i = -kTmHalo; i <= kTmHalo; ++i) {
                    const int s = centre + j * kTmLdsW + i;
                    const dn4 qc = s_col[s], qn = s_nrm[s];
                    if (__float_as_int(qc.w) == id && qn.w > 0.0f && ((i == 0 && j == 0) || dn_dot(qn.x, qn.y, qn.z, nx, ny, nz) >= a.cm)) {
                        S0 = S0 + 1.0f;
                        S1r = S1r + qc.x, S1g = S1g + qc.y, S1b = S1b + qc.z;
                        S2r = __builtin_fmaf(qc.x, qc.x, S2r), S2g = __builtin_fmaf(qc.y, qc.y, S2g), S2b = __builtin_fmaf(qc.z, qc.z, S2b);
                    }
                }
            vr = vg = vb = kDnVarCap;
            if (S0 >= m.mt) vr = tm_spatial_var(S0, S1r, S2r, W2), vg = tm_spatial_var(S0, S1g, S2g, W2), vb = tm_spatial_var(S0, S1b, S2b, W2);
        }
    }
    if (!inside) return; // (behind the last barrier)
    a.next.c[p] = dn4{or_, og, ob, No};
    a.next.v[p] = dn4{vr, vg, vb, 0.0f};
    a.next.g[p] = dn4{nx, ny, nz, __int_as_float(id)};
    a.next.p[p] = dn4{Px, Py, Pz, 0.0f};
    m.next_m[p] = dn4{qr, qg, qb, W2};
    a.rgb_out[3 * p] = or_, a.rgb_out[3 * p + 1] = og, a.rgb_out[3 * p + 2] = ob;
    a.var_out[3 * p] = vr, a.var_out[3 * p + 1] = vg, a.var_out[3 * p + 2] = vb;
    if (a.len_out) a.len_out[p] = No;
    if (m.w2_out) m.w2_out[p] = W2;
}

} // namespace rayz_dev_counts
