// temporal_modes_kernel.hpp — the device code of temporal accumulation's counts step (include/rayz_hip.h:
// rayz_hip_temporal_step_counts, rayz_hip_temporal_step_moments_counts), of its background mode (§4.27,
// rayz_hip_temporal_set_background) and of the plain step of its cubic resampling mode (§4.26, rayz_hip_temporal_set_resampling;
// tc_resample and the cubic moments kernel: temporal_cubic_kernel.hpp).  The host side: temporal.hpp, temporal_moments.hpp; the
// steps these are made from: temporal_kernel.hpp, temporal_moments_kernel.hpp.
//
// TWO bodies, each written once, and 17 kernels that are one call each.  ta_mode_step is the plain step (§4.15) and tm_mode_step the
// moments step (§4.16, without its feedback mode), through the same functions — ta_gather, ta_blend_head, ta_blend,
// tm_temporal_var, tm_spatial_var — and with what a mode changes behind compile-time flags:
//
//   COUNTS (§4.23)  the samples the current frame adds are a number per pixel, read from an array of height·width uint32, and may
//                   be 0 — a lattice frame (§4.21) samples one pixel in f², an adaptive frame (§4.14) as many as each pixel still
//                   needs.  A history record of length 0 holds no samples and is refused like a different surface (the gathers'
//                   LIVE flag); a pixel that got no sample and finds history keeps the gathered history, by selection, so that
//                   whatever its input holds — NaN included — reaches nothing; and the moments step's 7x7 neighbourhood counts only
//                   positions that were sampled: the count rides in the free lane of the staged normal record, so the LDS and the
//                   barriers are the scalar step's.  Per pixel 4 more bytes are read.  With every count equal to one spp >= 1 the
//                   step returns what the scalar step returns, bit for bit.
//   BG (§4.27)      a pixel whose centre ray misses the scene (id < 0) gathers history too.  A miss sees the sky at infinity, so
//                   where it lay in the previous frame depends only on how the view turned: the host gives the 3x3 matrix G that
//                   takes this frame's pixel centre (x, y, 1) to s·(x', y', 1) in the previous frame, and bg_gather runs §4.15's
//                   taps from there, accepting the history pixels that were misses themselves — no normal and no distance to
//                   compare.  Everything behind the sums is the hit pixel's arithmetic.  A pixel with id >= 0 takes ta_gather and
//                   is the INPUT-mode step bit for bit.  A wave with both kinds of lane runs both gathers, one after the other.
//   CUBIC (§4.26)   the plain step only, its moving form, and with neither of the other two: ta_gather keeps its four taps and,
//                   where tc_resample takes the sixteen around them, the colour is blended into its values; the variance and the
//                   length stay bilinear.  One byte per pixel says which.
//   CLIP (§4.28)    the moving step only, with one spp and bilinear taps: a pixel that found history clamps the history's colour,
//                   per channel, to mean ± g·sd of the CURRENT frame's 7x7 neighbourhood on the same surface (for a background
//                   pixel: of the misses in it) before the blend, and the moments step moves m2 with it.  The neighbourhood is
//                   §4.16 step 4's — tm_mode_stage and RAYZ_TM_TAPS below, which the moments step's spatial estimate runs too, so
//                   a pixel that takes both has one set of sums — and it needs the sums BEFORE the blend, so the vote and the
//                   staging come before the gather: a workgroup stages, once, where any of its pixels will look for history (in
//                   the moments step: or is a hit pixel, which may need the spatial estimate), and a pixel runs the taps between
//                   its gather and its blend.  The plain clip kernel therefore has the moments step's LDS and barriers, and no
//                   early return.  One byte per pixel says whether a channel was clipped.
//
// These are the kernels OUTSIDE the recorded set: temporal_step_kernel, tm_step and what they call are compiled from text that
// stays as it is, and the kernels here live in namespaces of their own, so that rayz_dev holds exactly the kernels
// it held.  Neither body is a symbol of its own: both are forced inline.
#pragma once

#include "temporal_cubic_kernel.hpp"

namespace rayz_dev {

struct TemporalModeArgs {
    TemporalArgs t;         // the plain step's arguments; with COUNTS, t.spp is not read
    float G[9];             // BG: this frame's pixel centre -> the previous frame's, up to scale (row-major; not read by a static step)
    const uint32_t* counts; // COUNTS: per pixel, the samples the current frame adds (never an output: a pixel reads its neighbours' too)
    uint8_t* taken;         // CUBIC: or NULL — one byte per pixel, 1 where the colour history came from the sixteen taps
};

struct TemporalMomentsModeArgs {
    TemporalMomentsArgs m; // the moments step's arguments; with COUNTS, m.t.spp is not read
    float G[9];
    const uint32_t* counts;
};

// CLIP (§4.28): what the clip kernels take beside their step's arguments.
struct TemporalClip {
    float g, mt;      // f32 of gamma and of the clip's own min_taps
    uint8_t* clipped; // or NULL — one byte per pixel, 1 where the clip changed a channel of the colour history
};

struct TemporalClipArgs {
    TemporalModeArgs m;
    TemporalClip k;
};

struct TemporalMomentsClipArgs {
    TemporalMomentsModeArgs m;
    TemporalClip k;
};

// §4.16 step 4's staging, by all 256 threads of a workgroup: the tile and its 3-pixel halo of the current frame, {r, g, b,
// bits(index)} and {n.x, n.y, n.z, count} per position — count: the position's own with COUNTS, else 1; 0 outside the frame.
template <bool COUNTS>
__device__ __forceinline__ void tm_mode_stage(const TemporalArgs& a, [[maybe_unused]] const uint32_t* counts, dn4* const s_col, dn4* const s_nrm) {
    const int bx = (int)(blockIdx.x * kDnTileW) - kTmHalo, by = (int)(blockIdx.y * kDnTileH) - kTmHalo;
    for (int t = (int)threadIdx.x; t < kTmLdsW * kTmLdsH; t += 256) { // (t < 532: inside both arrays)
        const int gx = bx + t % kTmLdsW, gy = by + t / kTmLdsW;
        dn4 vc{0.0f, 0.0f, 0.0f, __int_as_float(kTmOutside)}, vn{0.0f, 0.0f, 0.0f, 0.0f};
        if (gx >= 0 && gx < (int)a.width && gy >= 0 && gy < (int)a.height) { // (so q < width·height: inside counts too)
            const size_t q = (size_t)gy * a.width + (size_t)gx;
            vc = dn4{a.rgb[3 * q], a.rgb[3 * q + 1], a.rgb[3 * q + 2], __int_as_float(a.index[q])};
            vn = dn4{a.normal[3 * q], a.normal[3 * q + 1], a.normal[3 * q + 2], COUNTS ? (float)counts[q] : 1.0f};
        }
        s_col[t] = vc, s_nrm[t] = vn;
    }
}

// .. and its sums over the 49 staged positions around the thread's own (tx, ty), j outer and ascending: the ones on the pixel's
// surface (its index id, and the centre or a normal within cm of n; with COUNTS: sampled).  SKY (§4.28 rule 1): a pixel with
// id < 0 takes the positions inside the frame whose index is < 0 instead, with no normal to compare.
// A MACRO, and not a function as the staging is: the loop is written once, and every kernel that held it compiles it from the text
// it compiled it from — behind a call, even one forced inline, the compiler orders the loop's independent instructions differently,
// and the kernels outside §4.28 are to stay what they were.  It declares S0, S1r .. S2b (and centre) in the scope it stands in and
// reads a, s_col, s_nrm, tx, ty, id, nx, ny, nz and COUNTS from there: the static_asserts at its head name every one of them, so an
// expansion where one is missing, or is something else, does not compile.
#define RAYZ_TM_TAPS(SKY)                                                                                                                  \
    static_assert(std::is_same<std::decay_t<decltype(a)>, TemporalArgs>::value && std::is_same<std::decay_t<decltype(s_col)>, dn4*>::value &&   \
                      std::is_same<std::decay_t<decltype(s_nrm)>, dn4*>::value && std::is_same<std::decay_t<decltype(tx)>, int>::value &&       \
                      std::is_same<std::decay_t<decltype(ty)>, int>::value && std::is_same<std::decay_t<decltype(id)>, int32_t>::value &&       \
                      std::is_same<std::decay_t<decltype(nx)>, float>::value && std::is_same<std::decay_t<decltype(ny)>, float>::value &&       \
                      std::is_same<std::decay_t<decltype(nz)>, float>::value && std::is_same<std::decay_t<decltype(COUNTS)>, bool>::value,      \
                  "RAYZ_TM_TAPS reads a, s_col, s_nrm, tx, ty, id, nx, ny, nz and COUNTS of the scope it stands in");                      \
    float S0 = 0.0f, S1r = 0.0f, S1g = 0.0f, S1b = 0.0f, S2r = 0.0f, S2g = 0.0f, S2b = 0.0f;                                               \
    const int centre = (ty + kTmHalo) * kTmLdsW + tx + kTmHalo; /* taps: centre + j·38 + i stays within [0, 532) */                        \
    for (int j = -kTmHalo; j <= kTmHalo; ++j)                                                                                              \
        _Pragma("unroll") for (int i = -kTmHalo; i <= kTmHalo; ++i) {                                                                      \
            const int s = centre + j * kTmLdsW + i;                                                                                        \
            const dn4 qc = s_col[s], qn = s_nrm[s];                                                                                        \
            if ((SKY) && id < 0 ? __float_as_int(qc.w) < 0 && qn.w > 0.0f /* (a position outside the frame: count 0) */                    \
                                : __float_as_int(qc.w) == id && (!COUNTS || qn.w > 0.0f) &&                                                \
                                      ((i == 0 && j == 0) || dn_dot(qn.x, qn.y, qn.z, nx, ny, nz) >= a.cm)) {                              \
                S0 = S0 + 1.0f;                                                                                                            \
                S1r = S1r + qc.x, S1g = S1g + qc.y, S1b = S1b + qc.z;                                                                      \
                S2r = __builtin_fmaf(qc.x, qc.x, S2r), S2g = __builtin_fmaf(qc.y, qc.y, S2g), S2b = __builtin_fmaf(qc.z, qc.z, S2b);       \
            }                                                                                                                              \
        }

struct TmSums {
    float S0, S1r, S1g, S1b, S2r, S2g, S2b;
};

// A clip kernel's thread outside the frame takes the nearest coordinate inside it; every other thread and kernel its own.
template <bool CLIP> __device__ __forceinline__ int tm_clip_coord(int v, int n) { return CLIP && v >= n ? n - 1 : v; }

// §4.28 rule 2 for one channel: the history's mean h clamped to mu ± g·sd of the neighbourhood; hit: it lay outside.
__device__ __forceinline__ float tm_clip_channel(float S0, float S1, float S2, float g, float h, bool& hit) {
    const float mu = S1 / S0;
    const float d = S2 / S0 - mu * mu;
    const float dp = d > 0.0f ? d : 0.0f;
    const float e = g * __builtin_sqrtf((dp * S0) / (S0 - 1.0f));
    const float lo = mu - e, hi = mu + e;
    hit = h < lo || h > hi; // (a NaN h, or a NaN e: neither)
    return h < lo ? lo : (h > hi ? hi : h);
}

// .. for the three: h becomes hk where the neighbourhood has the clip's min_taps; returns the clipped channels' bits.
__device__ __forceinline__ uint32_t tm_clip(const TmSums& s, const TemporalClip& k, float (&h)[3]) {
    bool hit[3] = {false, false, false};
    if (s.S0 >= k.mt) {
        h[0] = tm_clip_channel(s.S0, s.S1r, s.S2r, k.g, h[0], hit[0]);
        h[1] = tm_clip_channel(s.S0, s.S1g, s.S2g, k.g, h[1], hit[1]);
        h[2] = tm_clip_channel(s.S0, s.S1b, s.S2b, k.g, h[2], hit[2]);
    }
    return (hit[0] ? 1u : 0u) | (hit[1] ? 2u : 0u) | (hit[2] ? 4u : 0u);
}

// §4.28 rule 4 for one channel: the history's second moment keeps its spread about the clipped mean.
__device__ __forceinline__ float tm_clip_m2(bool hit, float hq, float h, float hk) {
    const float t = hq - h * h;
    const float tp = t > 0.0f ? t : 0.0f;
    return hit ? __builtin_fmaf(hk, hk, tp) : hq;
}

// §4.27 rules 1 and 2 for one pixel (x, y) with id < 0 of a handle with history: the sums over the history taps that were misses.
// rec, R, STATIC, LIVE: as ta_gather's.
template <bool STATIC, int R, bool LIVE>
__device__ __forceinline__ TaAcc<R> bg_gather(const TemporalArgs& a, const float (&G)[9], const dn4* const* rec, size_t p, int x, int y) {
    TaAcc<R> acc;
    if (STATIC) {
        if (__float_as_int(a.prev.g[p].w) < 0) {
            dn4 own[R];
#pragma unroll
            for (int r = 0; r < R; ++r) own[r] = rec[r][p];
            if (!LIVE || own[0].w > 0.0f) acc.add(own, 1.0f);
        }
        return acc;
    }
    const float xf = (float)x, yf = (float)y;
    const float al = __builtin_fmaf(G[1], yf, __builtin_fmaf(G[0], xf, G[2]));
    const float be = __builtin_fmaf(G[4], yf, __builtin_fmaf(G[3], xf, G[5]));
    const float ga = __builtin_fmaf(G[7], yf, __builtin_fmaf(G[6], xf, G[8]));
    if (!(ga > 0.0f)) return acc;
    const float hx = al / ga, hy = be / ga;
    if (!(hx > -1.0f && hx < (float)a.width && hy > -1.0f && hy < (float)a.height)) return acc; // (so the casts below are in range)
    const float x0 = __builtin_floorf(hx), y0 = __builtin_floorf(hy);
    const float fx = hx - x0, fy = hy - y0;
    const int ix = (int)x0, iy = (int)y0;
    // Two rounds of loads, as ta_gather's: every tap's index (the .w of its guide record; the point records are not read), then the
    // records it adds.  A tap outside the frame loads the nearest pixel inside it (a valid address) and is refused.
    size_t q[4];
    bool ok[4];
    float gw[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int qx = ix + (t & 1), qy = iy + (t >> 1);
        ok[t] = qx >= 0 && qx < (int)a.width && qy >= 0 && qy < (int)a.height;
        const int cx = qx < 0 ? 0 : (qx >= (int)a.width ? (int)a.width - 1 : qx);
        const int cy = qy < 0 ? 0 : (qy >= (int)a.height ? (int)a.height - 1 : qy);
        q[t] = (size_t)cy * a.width + (size_t)cx;
        gw[t] = a.prev.g[q[t]].w;
    }
    dn4 tap[4][R];
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        ok[t] = ok[t] && __float_as_int(gw[t]) < 0;
#pragma unroll
        for (int r = 0; r < R; ++r) tap[t][r] = rec[r][q[t]];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) // j outer, i inner: t = 2·j + i
        if (ok[t] && (!LIVE || tap[t][0].w > 0.0f)) acc.add(tap[t], ((t & 1) ? fx : 1.0f - fx) * ((t >> 1) ? fy : 1.0f - fy));
    return acc;
}

// §4.15's step with the modes' flags: temporal_step_kernel's body (temporal_kernel.hpp) with n for spp, the gather chosen by the
// pixel's kind and the history's colour from tc_resample where that takes the sixteen taps.
// CLIP (§4.28; k, s_col, s_nrm: its parameters and the kernel's two LDS arrays): the kernel has the moments step's barriers, which
// all 256 threads reach — a thread outside the frame loads, votes and gathers for the nearest pixel inside it (one of its own tile,
// so the vote is the tile's), runs the taps around its OWN position in the staged tile (inside the LDS arrays, and of no meaning)
// and stores nothing — and they come BEFORE the gather: a workgroup in which any pixel will look for history
// stages, and a pixel that finds it runs the taps between the blend's head and the blend.
template <bool STATIC, bool COUNTS, bool BG, bool CUBIC, bool CLIP = false>
__device__ __forceinline__ void ta_mode_step(const TemporalModeArgs& ma, [[maybe_unused]] const TemporalClip* k = nullptr,
                                             [[maybe_unused]] dn4* const s_col = nullptr, [[maybe_unused]] dn4* const s_nrm = nullptr) {
    static_assert(!(CUBIC && (STATIC || COUNTS || BG)), "the cubic path is the moving plain step's, with one spp and no background history");
    static_assert(!(CLIP && (STATIC || COUNTS || CUBIC)), "the clip is the moving step's, with one spp and bilinear taps");
    const TemporalArgs& a = ma.t;
    const int x = tm_clip_coord<CLIP>((int)(blockIdx.x * kDnTileW + threadIdx.x % kDnTileW), (int)a.width);
    const int y = tm_clip_coord<CLIP>((int)(blockIdx.y * kDnTileH + threadIdx.x / kDnTileW), (int)a.height);
    if (!CLIP && (x >= (int)a.width || y >= (int)a.height)) return;
    const size_t p = (size_t)y * a.width + (size_t)x;
    const float cr = a.rgb[3 * p], cg = a.rgb[3 * p + 1], cb = a.rgb[3 * p + 2];
    const float sr = dn_clamp_var(a.var[3 * p]), sg = dn_clamp_var(a.var[3 * p + 1]), sb = dn_clamp_var(a.var[3 * p + 2]);
    const int32_t id = a.index[p];
    const float nx = a.normal[3 * p], ny = a.normal[3 * p + 1], nz = a.normal[3 * p + 2];
    const float Px = a.point[3 * p], Py = a.point[3 * p + 1], Pz = a.point[3 * p + 2];
    const float n = COUNTS ? (float)ma.counts[p] : a.spp;
    float or_ = cr, og = cg, ob = cb, vr = sr, vg = sg, vb = sb, No = n; // no history: the input, by selection
    [[maybe_unused]] bool took = false;
    [[maybe_unused]] uint32_t hit = 0; // CLIP: the clipped channels' bits
    if constexpr (CLIP) {              // the vote: reached by every thread; its result is the same in all of them
        if (__syncthreads_or((BG || id >= 0) && a.has_history ? 1 : 0)) {
            tm_mode_stage<false>(a, nullptr, s_col, s_nrm);
            __syncthreads(); // all 256 threads are here: the branch is the workgroup's, not a thread's
        }
    }
    if ((BG || id >= 0) && a.has_history) {
        const dn4* const rec[2] = {a.prev.c, a.prev.v};
        typename std::conditional<CUBIC, TaTaps<2>, TaNoTaps>::type keep; // (where ta_gather leaves its taps, or nothing)
        TaAcc<2> acc;
        if (!BG || id >= 0)
            acc = ta_gather<STATIC, 2, COUNTS>(a, rec, p, id, nx, ny, nz, Px, Py, Pz, &keep);
        else if constexpr (BG)
            acc = bg_gather<STATIC, 2, COUNTS>(a, ma.G, rec, p, x, y);
        if (acc.found()) {
            const TaBlend h = ta_blend_head(acc, a, n);
            No = h.N; // (n = 0: hN + 0, capped)
            if (!COUNTS || n > 0.0f) {
                const float a2 = h.al * h.al, k2 = h.k * h.k;
                if constexpr (CUBIC) { // the history's colour: the bilinear means, or tc_resample's values
                    float hc[1][3] = {{acc.mean(0, 0), acc.mean(0, 1), acc.mean(0, 2)}};
                    took = tc_resample<1>(a, rec, keep, id, nx, ny, nz, Px, Py, Pz, hc);
                    or_ = ta_blend(h.al, cr, hc[0][0]), og = ta_blend(h.al, cg, hc[0][1]), ob = ta_blend(h.al, cb, hc[0][2]);
                } else if constexpr (CLIP) { // .. or the means clamped to the box of the current frame's neighbourhood
                    const int tx = (int)(threadIdx.x % kDnTileW), ty = (int)(threadIdx.x / kDnTileW);
                    RAYZ_TM_TAPS(BG)
                    float hc[3] = {acc.mean(0, 0), acc.mean(0, 1), acc.mean(0, 2)};
                    hit = tm_clip(TmSums{S0, S1r, S1g, S1b, S2r, S2g, S2b}, *k, hc);
                    or_ = ta_blend(h.al, cr, hc[0]), og = ta_blend(h.al, cg, hc[1]), ob = ta_blend(h.al, cb, hc[2]);
                } else {
                    or_ = ta_blend(h.al, cr, acc.mean(0, 0));
                    og = ta_blend(h.al, cg, acc.mean(0, 1));
                    ob = ta_blend(h.al, cb, acc.mean(0, 2));
                }
                vr = __builtin_fmaf(a2, sr, k2 * acc.mean(1, 0));
                vg = __builtin_fmaf(a2, sg, k2 * acc.mean(1, 1));
                vb = __builtin_fmaf(a2, sb, k2 * acc.mean(1, 2));
            } else { // no sample: the gathered history, by selection — the input is loaded and never used
                or_ = acc.mean(0, 0), og = acc.mean(0, 1), ob = acc.mean(0, 2);
                vr = acc.mean(1, 0), vg = acc.mean(1, 1), vb = acc.mean(1, 2);
            }
        }
    }
    if constexpr (CLIP) // (behind the last barrier: a thread outside the frame has no pixel of its own)
        if (blockIdx.x * kDnTileW + threadIdx.x % kDnTileW >= a.width || blockIdx.y * kDnTileH + threadIdx.x / kDnTileW >= a.height) return;
    a.next.c[p] = dn4{or_, og, ob, No};
    a.next.v[p] = dn4{vr, vg, vb, 0.0f};
    a.next.g[p] = dn4{nx, ny, nz, __int_as_float(id)};
    a.next.p[p] = dn4{Px, Py, Pz, 0.0f};
    a.rgb_out[3 * p] = or_, a.rgb_out[3 * p + 1] = og, a.rgb_out[3 * p + 2] = ob;
    a.var_out[3 * p] = vr, a.var_out[3 * p + 1] = vg, a.var_out[3 * p + 2] = vb;
    if (a.len_out) a.len_out[p] = No;
    if constexpr (CUBIC)
        if (ma.taken) ma.taken[p] = took ? 1 : 0;
    if constexpr (CLIP)
        if (k->clipped) k->clipped[p] = hit ? 1 : 0;
}

// §4.16's step with the modes' flags: tm_step's body (temporal_moments_kernel.hpp) without its feedback and cubic modes, with n for
// spp, the gather chosen by the pixel's kind and the neighbourhood over sampled positions.  The barriers are tm_step's — the vote
// and the barrier behind the staging are reached by all 256 threads, a thread outside the frame skips only the per-pixel work and
// the stores — and so is the LDS: two arrays of 38 x 14 records and the vote's.  A background pixel never votes for the staging:
// its variance is the temporal one where it found history that is long enough, and +0 elsewhere (§4.27 rule 3; without BG a miss
// gathers nothing, found stays false, and the rule is §4.16's: +0).
// CLIP (§4.28; k: its parameters): the vote and the staging come BEFORE the gather — a workgroup with a hit pixel, or with a
// background pixel that will look for history, stages — and a pixel that finds history, or is a hit pixel, runs the taps once
// behind the gather: the clip takes their sums between the blend's head and the blend, and the spatial estimate takes the same.
template <bool STATIC, bool COUNTS, bool BG, bool CLIP = false>
__device__ __forceinline__ void tm_mode_step(const TemporalMomentsModeArgs& ma, dn4* const s_col, dn4* const s_nrm,
                                             [[maybe_unused]] const TemporalClip* k = nullptr) {
    static_assert(!(CLIP && (STATIC || COUNTS)), "the clip is the moving step's, with one spp");
    const TemporalMomentsArgs& m = ma.m;
    const TemporalArgs& a = m.t;
    const int tx = (int)(threadIdx.x % kDnTileW), ty = (int)(threadIdx.x / kDnTileW);
    const int x = (int)(blockIdx.x * kDnTileW) + tx, y = (int)(blockIdx.y * kDnTileH) + ty;
    const bool inside = x < (int)a.width && y < (int)a.height; // NO early return: every thread reaches the vote and the barrier
    const size_t p = inside ? (size_t)y * a.width + (size_t)x : 0;
    float nx = 0.0f, ny = 0.0f, nz = 0.0f, Px = 0.0f, Py = 0.0f, Pz = 0.0f;
    float or_ = 0.0f, og = 0.0f, ob = 0.0f, No = 0.0f, qr = 0.0f, qg = 0.0f, qb = 0.0f, W2 = 1.0f, vr = 0.0f, vg = 0.0f, vb = 0.0f;
    int32_t id = -1;
    bool spatial = false;
    [[maybe_unused]] uint32_t hit = 0; // CLIP: the clipped channels' bits
    [[maybe_unused]] TmSums sums{};    // CLIP: the neighbourhood's, of a hit pixel or one that found history
    if constexpr (CLIP) {              // the vote: reached by every thread; its result is the same in all of them
        const int32_t vid = inside ? a.index[p] : -1;
        if (__syncthreads_or(inside && (vid >= 0 || (BG && a.has_history)) ? 1 : 0)) {
            tm_mode_stage<false>(a, nullptr, s_col, s_nrm);
            __syncthreads(); // all 256 threads are here: the branch is the workgroup's, not a thread's
        }
    }
    if (inside) {
        const float cr = a.rgb[3 * p], cg = a.rgb[3 * p + 1], cb = a.rgb[3 * p + 2];
        const float n = COUNTS ? (float)ma.counts[p] : a.spp;
        id = a.index[p];
        nx = a.normal[3 * p], ny = a.normal[3 * p + 1], nz = a.normal[3 * p + 2];
        Px = a.point[3 * p], Py = a.point[3 * p + 1], Pz = a.point[3 * p + 2];
        or_ = cr, og = cg, ob = cb, No = n;                  // no history: the input, by selection ..
        qr = cr * cr, qg = cg * cg, qb = cb * cb, W2 = 1.0f; // .. its square, and the weight of one frame
        bool found = false;
        if ((BG || id >= 0) && a.has_history) {
            const dn4* const rec[2] = {a.prev.c, m.prev_m};
            TaAcc<2> acc;
            if (!BG || id >= 0)
                acc = ta_gather<STATIC, 2, COUNTS>(a, rec, p, id, nx, ny, nz, Px, Py, Pz);
            else if constexpr (BG)
                acc = bg_gather<STATIC, 2, COUNTS>(a, ma.G, rec, p, x, y);
            found = acc.found();
            if constexpr (CLIP)
                if (id >= 0 || found) {
                    RAYZ_TM_TAPS(BG)
                    sums = TmSums{S0, S1r, S1g, S1b, S2r, S2g, S2b};
                }
            if (found) {
                const TaBlend h = ta_blend_head(acc, a, n);
                No = h.N; // (n = 0: hN + 0, capped)
                if constexpr (CLIP) { // the history's colour clamped to the neighbourhood's box, and m2 moved with it
                    const float h0[3] = {acc.mean(0, 0), acc.mean(0, 1), acc.mean(0, 2)};
                    float hc[3] = {h0[0], h0[1], h0[2]};
                    hit = tm_clip(sums, *k, hc);
                    or_ = ta_blend(h.al, cr, hc[0]), og = ta_blend(h.al, cg, hc[1]), ob = ta_blend(h.al, cb, hc[2]);
                    qr = ta_blend(h.al, cr * cr, tm_clip_m2(hit & 1u, acc.mean(1, 0), h0[0], hc[0]));
                    qg = ta_blend(h.al, cg * cg, tm_clip_m2(hit & 2u, acc.mean(1, 1), h0[1], hc[1]));
                    qb = ta_blend(h.al, cb * cb, tm_clip_m2(hit & 4u, acc.mean(1, 2), h0[2], hc[2]));
                    W2 = __builtin_fmaf(h.k * h.k, acc.mean(1, 3), h.al * h.al);
                } else if (!COUNTS || n > 0.0f) {
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
        if (id >= 0 ? !spatial : (found && !(W2 > m.wm)))
            vr = tm_temporal_var(qr, or_, W2), vg = tm_temporal_var(qg, og, W2), vb = tm_temporal_var(qb, ob, W2);
    }
    // The vote: reached by every thread of the workgroup; its result is the same in all of them.  (CLIP: it is behind us.)
    if (CLIP || __syncthreads_or(spatial ? 1 : 0)) {
        if constexpr (!CLIP) {
            tm_mode_stage<COUNTS>(a, ma.counts, s_col, s_nrm);
            __syncthreads(); // all 256 threads are here: the branch is the workgroup's, not a thread's
        }
        if (spatial) {
            TmSums s = sums; // (CLIP: the ones the clip took)
            if constexpr (!CLIP) {
                RAYZ_TM_TAPS(false)
                s = TmSums{S0, S1r, S1g, S1b, S2r, S2g, S2b};
            }
            vr = vg = vb = kDnVarCap;
            if (s.S0 >= m.mt) vr = tm_spatial_var(s.S0, s.S1r, s.S2r, W2), vg = tm_spatial_var(s.S0, s.S1g, s.S2g, W2), vb = tm_spatial_var(s.S0, s.S1b, s.S2b, W2);
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
    if constexpr (CLIP)
        if (k->clipped) k->clipped[p] = hit ? 1 : 0;
}

} // namespace rayz_dev

// The kernels live in namespaces of their own: the kernels of rayz_dev are a recorded set (tests/test_slab_cells_isa.py).
namespace rayz_dev_counts {
using namespace rayz_dev;

template <bool STATIC> __global__ __launch_bounds__(256) void temporal_counts_kernel(const TemporalModeArgs a) {
    ta_mode_step<STATIC, true, false, false>(a);
}

template <bool STATIC> __global__ __launch_bounds__(256) void temporal_counts_moments_kernel(const TemporalMomentsModeArgs a) {
    __shared__ dn4 s_col[kTmLdsH * kTmLdsW], s_nrm[kTmLdsH * kTmLdsW];
    tm_mode_step<STATIC, true, false>(a, s_col, s_nrm);
}

} // namespace rayz_dev_counts

// {plain, moments} x {one spp, a count per pixel} x {static, moving}
namespace rayz_dev_bg {
using namespace rayz_dev;

template <bool STATIC> __global__ __launch_bounds__(256) void temporal_bg_kernel(const TemporalModeArgs a) {
    ta_mode_step<STATIC, false, true, false>(a);
}

template <bool STATIC> __global__ __launch_bounds__(256) void temporal_bg_counts_kernel(const TemporalModeArgs a) {
    ta_mode_step<STATIC, true, true, false>(a);
}

template <bool STATIC> __global__ __launch_bounds__(256) void temporal_bg_moments_kernel(const TemporalMomentsModeArgs a) {
    __shared__ dn4 s_col[kTmLdsH * kTmLdsW], s_nrm[kTmLdsH * kTmLdsW];
    tm_mode_step<STATIC, false, true>(a, s_col, s_nrm);
}

template <bool STATIC> __global__ __launch_bounds__(256) void temporal_bg_counts_moments_kernel(const TemporalMomentsModeArgs a) {
    __shared__ dn4 s_col[kTmLdsH * kTmLdsW], s_nrm[kTmLdsH * kTmLdsW];
    tm_mode_step<STATIC, true, true>(a, s_col, s_nrm);
}

} // namespace rayz_dev_bg

namespace rayz_dev_cubic {

// The plain step's moving form (temporal_step_kernel<false>, whose body stays as it is) with the colour history from tc_resample.
__global__ __launch_bounds__(256) void temporal_cubic_step_kernel(const TemporalModeArgs a) {
    ta_mode_step<false, false, false, true>(a);
}

} // namespace rayz_dev_cubic

// §4.28: {plain, moments} x {background input, accumulate}, the moving step only.  All four have the moments step's LDS.
namespace rayz_dev_clip {
using namespace rayz_dev;

template <bool BG> __global__ __launch_bounds__(256) void clip_plain_kernel(const TemporalClipArgs a) {
    __shared__ dn4 s_col[kTmLdsH * kTmLdsW], s_nrm[kTmLdsH * kTmLdsW];
    ta_mode_step<false, false, BG, false, true>(a.m, &a.k, s_col, s_nrm);
}

template <bool BG> __global__ __launch_bounds__(256) void clip_moments_kernel(const TemporalMomentsClipArgs a) {
    __shared__ dn4 s_col[kTmLdsH * kTmLdsW], s_nrm[kTmLdsH * kTmLdsW];
    tm_mode_step<false, false, BG, true>(a.m, s_col, s_nrm, &a.k);
}

} // namespace rayz_dev_clip

#undef RAYZ_TM_TAPS
