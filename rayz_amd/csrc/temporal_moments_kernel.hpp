// temporal_moments_kernel.hpp — the device code of temporal accumulation's moments mode (include/rayz_hip.h:
// rayz_hip_temporal_step_moments; the handle and the validation: temporal_moments.hpp; the plain step: temporal_kernel.hpp).
//
// ONE launch per step, as the plain step: 32x8 tiles, 256 threads, the taps in two rounds of loads.  The colour and the length are
// the plain step's, operation for operation (§4.15 steps 1-4: temporal_kernel.hpp's ta_gather, ta_blend_head and ta_blend, called
// here with this mode's records); the variance comes from the history instead of from the caller: a
// fifth record per pixel, {m2.r, m2.g, m2.b, W2}, carries the second moment of the colour under the same blend and the sum of the
// squared frame weights, and v = max(m2 − c², 0)·W2 / (1 − W2).  Where the history is too short to say anything (W2 > w2_max: a
// first frame, a disocclusion) the variance is estimated over the CURRENT frame's 7x7 neighbourhood on the same surface.
//
// That neighbourhood is the only part that reads other pixels of the current frame, and the only part that uses LDS: every thread
// first finishes its pixel's temporal part and learns whether it needs the spatial estimate, the workgroup votes, and only a
// workgroup with at least one such pixel stages its tile plus a 3-pixel halo (38x14 positions of {r, g, b, bits(index)} and
// {n.x, n.y, n.z, 0}: 17,024 bytes) and runs the 49 taps from there.  A workgroup whose history is settled costs the plain step plus
// one record each way.
//
// THE BARRIERS: the vote and the barrier behind the staging are reached by all 256 threads of a workgroup, always.  A thread whose
// pixel lies outside the frame does not return early as the plain kernel's does: it votes "no", helps to stage, and skips only the
// per-pixel work and the stores.  The staging branch is taken by a whole workgroup or by none (the vote's result is the same in
// every thread), so the barrier inside it is not under divergent control flow.
//
// The step's body is ONE function, tm_step<STATIC, FEEDBACK>: the two kernels here instantiate it with FEEDBACK = false, the
// feedback handle's two (temporal_feedback_kernel.hpp, §4.17) with true — there every accepted tap also reads the history's raw first
// moment m1 from the v record, and step 3 takes the variance from it instead of from the colour, which may be a fed-back one.
#pragma once

#include "temporal_kernel.hpp"

namespace rayz_dev {

constexpr int kTmHalo = 3;                                                    // the spatial estimate's taps: −3 .. 3 on both axes
constexpr int kTmLdsW = kDnTileW + 2 * kTmHalo, kTmLdsH = kDnTileH + 2 * kTmHalo; // 38 x 14 staged positions
constexpr int kTmOutside = (int)0x80000000;                                   // the index of a staged position outside the frame: equals no id >= 0

struct TemporalMomentsArgs {
    TemporalArgs t;    // the plain step's arguments; t.var is not read, t.var_out receives v_out, t.prev.v is not read (the feedback
                       // step, §4.17: t.prev.v and t.next.v hold {m1.r, m1.g, m1.b, 0}, the raw first moment)
    const dn4* prev_m; // per pixel {m2.r, m2.g, m2.b, W2}: the history's second moment and its sum of squared frame weights
    dn4* next_m;
    float* w2_out;     // or NULL
    float wm, mt;      // f32 of w2_max and min_taps
};

// §4.16 step 3 for one channel: the variance of the accumulated mean from its second moment.
__device__ __forceinline__ float tm_temporal_var(float m2, float c, float W2) {
    const float e = m2 - (c * c);
    const float ep = e > 0.0f ? e : 0.0f;
    return dn_clamp_var((ep * W2) / (1.0f - W2));
}

// §4.16 step 4 for one channel, behind the sums: the unbiased sample variance of the neighbourhood, scaled to the mean's weight.
__device__ __forceinline__ float tm_spatial_var(float S0, float S1, float S2, float W2) {
    const float mu = S1 / S0;
    const float d = S2 / S0 - mu * mu;
    const float dp = d > 0.0f ? d : 0.0f;
    return dn_clamp_var(((dp * S0) / (S0 - 1.0f)) * W2);
}

// §4.26 (temporal_cubic_kernel.hpp): the colour (NC = 2: and the second record's three channels) of a pixel that found history,
// from the sixteen taps around the four that ta_gather kept in k — h[r][ch], where the answer is true.
template <int NC>
__device__ __forceinline__ bool tc_resample(const TemporalArgs& a, const dn4* const* rec, const TaTaps<2>& k, int32_t id, float nx,
                                            float ny, float nz, float Px, float Py, float Pz, float (&h)[NC][3]);

// A cubic step's state of one pixel: the taps ta_gather kept, whether the sixteen were taken, and where to say so (or NULL).
struct TcPixel {
    TaTaps<2> keep;
    bool took = false;
    uint8_t* taken;
};

// Where ta_gather leaves its taps: in a cubic step's state, or nowhere.
__device__ __forceinline__ TaTaps<2>* tm_keep(TcPixel* tc) { return &tc->keep; }
__device__ __forceinline__ TaNoTaps* tm_keep(TaNoTaps*) { return nullptr; }

// The step of one workgroup; s_col and s_nrm: the kernel's two LDS arrays of kTmLdsH·kTmLdsW records.
// Cubic = TcPixel (§4.26; the moving form without feedback): ta_gather keeps its taps in *tc, and where tc_resample takes the
// sixteen taps the colour and m2 are blended into its values instead.
template <bool STATIC, bool FEEDBACK, class Cubic = TaNoTaps>
__device__ __forceinline__ void tm_step(const TemporalMomentsArgs& m, dn4* const s_col, dn4* const s_nrm,
                                        [[maybe_unused]] Cubic* tc = nullptr) {
    constexpr bool CUBIC = std::is_same<Cubic, TcPixel>::value;
    static_assert(!(CUBIC && (STATIC || FEEDBACK)), "the cubic path is the moving moments step's");
    const TemporalArgs& a = m.t;
    const int tx = (int)(threadIdx.x % kDnTileW), ty = (int)(threadIdx.x / kDnTileW);
    const int x = (int)(blockIdx.x * kDnTileW) + tx, y = (int)(blockIdx.y * kDnTileH) + ty;
    const bool inside = x < (int)a.width && y < (int)a.height; // NO early return: every thread reaches the vote and the barrier
    const size_t p = inside ? (size_t)y * a.width + (size_t)x : 0;
    float cr = 0.0f, cg = 0.0f, cb = 0.0f, nx = 0.0f, ny = 0.0f, nz = 0.0f, Px = 0.0f, Py = 0.0f, Pz = 0.0f;
    float or_ = 0.0f, og = 0.0f, ob = 0.0f, No = 0.0f, qr = 0.0f, qg = 0.0f, qb = 0.0f, W2 = 1.0f, vr = 0.0f, vg = 0.0f, vb = 0.0f;
    float fr = 0.0f, fg = 0.0f, fb = 0.0f; // FEEDBACK: m1', the raw first moment
    int32_t id = -1;
    bool spatial = false;
    if (inside) {
        cr = a.rgb[3 * p], cg = a.rgb[3 * p + 1], cb = a.rgb[3 * p + 2];
        id = a.index[p];
        nx = a.normal[3 * p], ny = a.normal[3 * p + 1], nz = a.normal[3 * p + 2];
        Px = a.point[3 * p], Py = a.point[3 * p + 1], Pz = a.point[3 * p + 2];
        or_ = cr, og = cg, ob = cb, No = a.spp;              // no history: the input, by selection ..
        qr = cr * cr, qg = cg * cg, qb = cb * cb, W2 = 1.0f; // .. its square, and the weight of one frame
        fr = cr, fg = cg, fb = cb;
        if (id >= 0 && a.has_history) {
            // §4.15 steps 1-4 (temporal_kernel.hpp): the taps add the colour + length and moment records and, in the feedback
            // step, the raw first moment, which the v record holds there.
            constexpr int R = FEEDBACK ? 3 : 2;
            const dn4* const rec[3] = {a.prev.c, m.prev_m, a.prev.v};
            const TaAcc<R> acc = ta_gather<STATIC, R>(a, rec, p, id, nx, ny, nz, Px, Py, Pz, tm_keep(tc));
            if (acc.found()) {
                const TaBlend h = ta_blend_head(acc, a);
                if constexpr (CUBIC) { // the history's colour and m2: the bilinear means, or tc_resample's values
                    float hc[2][3] = {{acc.mean(0, 0), acc.mean(0, 1), acc.mean(0, 2)}, {acc.mean(1, 0), acc.mean(1, 1), acc.mean(1, 2)}};
                    tc->took = tc_resample<2>(a, rec, tc->keep, id, nx, ny, nz, Px, Py, Pz, hc);
                    or_ = ta_blend(h.al, cr, hc[0][0]), og = ta_blend(h.al, cg, hc[0][1]), ob = ta_blend(h.al, cb, hc[0][2]);
                    qr = ta_blend(h.al, cr * cr, hc[1][0]), qg = ta_blend(h.al, cg * cg, hc[1][1]), qb = ta_blend(h.al, cb * cb, hc[1][2]);
                } else {
                    or_ = ta_blend(h.al, cr, acc.mean(0, 0));
                    og = ta_blend(h.al, cg, acc.mean(0, 1));
                    ob = ta_blend(h.al, cb, acc.mean(0, 2));
                    qr = ta_blend(h.al, cr * cr, acc.mean(1, 0));
                    qg = ta_blend(h.al, cg * cg, acc.mean(1, 1));
                    qb = ta_blend(h.al, cb * cb, acc.mean(1, 2));
                }
                W2 = __builtin_fmaf(h.k * h.k, acc.mean(1, 3), h.al * h.al);
                if constexpr (FEEDBACK) {
                    fr = ta_blend(h.al, cr, acc.mean(2, 0));
                    fg = ta_blend(h.al, cg, acc.mean(2, 1));
                    fb = ta_blend(h.al, cb, acc.mean(2, 2));
                }
                No = h.N;
            }
        }
        spatial = id >= 0 && W2 > m.wm;
        if (id >= 0 && !spatial) { // (the feedback step: from the raw first moment, whatever colour was fed back)
            vr = tm_temporal_var(qr, FEEDBACK ? fr : or_, W2);
            vg = tm_temporal_var(qg, FEEDBACK ? fg : og, W2);
            vb = tm_temporal_var(qb, FEEDBACK ? fb : ob, W2);
        }
    }
    // The vote: reached by every thread of the workgroup; its result is the same in all of them.
    if (__syncthreads_or(spatial ? 1 : 0)) {
        const int bx = (int)(blockIdx.x * kDnTileW) - kTmHalo, by = (int)(blockIdx.y * kDnTileH) - kTmHalo;
        for (int t = (int)threadIdx.x; t < kTmLdsW * kTmLdsH; t += 256) { // (t < 532: inside both arrays)
            const int gx = bx + t % kTmLdsW, gy = by + t / kTmLdsW;
            dn4 vc{0.0f, 0.0f, 0.0f, __int_as_float(kTmOutside)}, vn{0.0f, 0.0f, 0.0f, 0.0f};
            if (gx >= 0 && gx < (int)a.width && gy >= 0 && gy < (int)a.height) {
                const size_t q = (size_t)gy * a.width + (size_t)gx;
                vc = dn4{a.rgb[3 * q], a.rgb[3 * q + 1], a.rgb[3 * q + 2], __int_as_float(a.index[q])};
                vn = dn4{a.normal[3 * q], a.normal[3 * q + 1], a.normal[3 * q + 2], 0.0f};
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
                    if (__float_as_int(qc.w) == id && ((i == 0 && j == 0) || dn_dot(qn.x, qn.y, qn.z, nx, ny, nz) >= a.cm)) {
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
    a.next.v[p] = FEEDBACK ? dn4{fr, fg, fb, 0.0f} : dn4{vr, vg, vb, 0.0f};
    a.next.g[p] = dn4{nx, ny, nz, __int_as_float(id)};
    a.next.p[p] = dn4{Px, Py, Pz, 0.0f};
    m.next_m[p] = dn4{qr, qg, qb, W2};
    a.rgb_out[3 * p] = or_, a.rgb_out[3 * p + 1] = og, a.rgb_out[3 * p + 2] = ob;
    a.var_out[3 * p] = vr, a.var_out[3 * p + 1] = vg, a.var_out[3 * p + 2] = vb;
    if (a.len_out) a.len_out[p] = No;
    if (m.w2_out) m.w2_out[p] = W2;
    if constexpr (CUBIC)
        if (tc->taken) tc->taken[p] = tc->took ? 1 : 0;
}

template <bool STATIC> __global__ __launch_bounds__(256) void temporal_moments_step_kernel(const TemporalMomentsArgs m) {
    __shared__ dn4 s_col[kTmLdsH * kTmLdsW], s_nrm[kTmLdsH * kTmLdsW];
    tm_step<STATIC, false>(m, s_col, s_nrm);
}

} // namespace rayz_dev
