// denoise.hpp — the G-buffer-guided à-trous denoiser's device code (include/rayz_hip.h: rayz_hip_denoiser_*).
//
// An image-space filter on whole f32 frames: a PACK pass turns the caller's radiance and camera-query G-buffer into 16-byte
// aligned per-pixel records once (the guides do not change between levels), then ONE launch per level reads a colour buffer
// and writes the other, 25 taps at stride 2^l; the last level multiplies the albedo back in and writes packed RGB.
//
// The arithmetic is a contract (§4.11): + - x, the FMAs written below, correctly rounded divides, comparisons — nothing else,
// so that tests/denoise_mirror.cpp restates it bit for bit.  Everything a tap computes is in dn_tap(); both level kernels call it
// with the taps in the same order (j outer, i inner, ascending), so the staging a level uses never changes a value.
//
// Guides are FIRST-HIT guides: a mirror or a glass ball is filtered by its own surface's normal and point, not by what it
// reflects or refracts — the reflection in it is smoothed as if it were a texture of the ball.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace rayz_dev {

typedef float dn4 __attribute__((ext_vector_type(4)));

constexpr int kDnTileW = 32, kDnTileH = 8;  // output pixels of a workgroup: 256 threads, a wave covers two tile rows
constexpr int kDnMaxLdsLog2 = 2;            // the LDS form exists for strides 1, 2, 4 (halo 2·s on every side)
constexpr int kDnLdsMaxStride = 2;          // levels up to this stride use it, wider ones read global memory: measured, DESIGN.md §6
                                            // (RAYZ_DEBUG_DENOISE_LDS_STRIDE overrides it for measurement)

struct DenoiseArgs {
    const dn4* __restrict__ ga;   // per pixel {n.x, n.y, n.z, bg ? 1 : 0}
    const dn4* __restrict__ gb;   // per pixel {P.x, P.y, P.z, 0}
    const dn4* __restrict__ mod;  // per pixel {m.r, m.g, m.b, 0}: read by the last level only
    const dn4* __restrict__ src;  // this level's colours {e.r, e.g, e.b, 0}
    dn4* __restrict__ dst;        // next level's colours (not the last level)
    float* __restrict__ rgb;      // packed RGB out (the last level)
    uint32_t width, height;
    int stride;                   // 2^l
    uint32_t normal_power_log2;
    float sp2;                    // f32(sigma_plane) x f32(sigma_plane)
    float sc2;                    // f32(sigma_color) x f32(sigma_color); +inf switches the colour term off exactly
    float cl;                     // 4^l
};

__device__ __forceinline__ float dn_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx)); // fma(z, z', fma(y, y', x·x')): the order §4.11 states
}
__device__ __forceinline__ float dn_max0(float x) { return x > 0.0f ? x : 0.0f; } // (a NaN gives 0)

struct DnAcc {
    float W, r, g, b;
};

// One tap: centre pixel (pa, pb, pc), tap pixel (qa, qb, qc), h = k[i]·k[j].
__device__ __forceinline__ void dn_tap(const dn4 pa, const dn4 pb, const dn4 pc, const dn4 qa, const dn4 qb, const dn4 qc,
                                       const float h, const DenoiseArgs& a, DnAcc& acc) {
    const bool bgp = pa.w != 0.0f, bgq = qa.w != 0.0f;
    float g = 1.0f;
    if (bgp || bgq) {
        if (!(bgp && bgq)) return; // background never mixes with a hit: the tap is skipped, as one outside the frame is
    } else {
        float wn = dn_max0(dn_dot(pa.x, pa.y, pa.z, qa.x, qa.y, qa.z));
        for (uint32_t k = 0; k < a.normal_power_log2; ++k) wn = wn * wn;
        const float vx = qb.x - pb.x, vy = qb.y - pb.y, vz = qb.z - pb.z;
        const float d2 = dn_dot(vx, vy, vz, vx, vy, vz);
        const float pl = dn_dot(pa.x, pa.y, pa.z, vx, vy, vz);
        float wz = 1.0f;
        if (d2 != 0.0f) {
            const float u = dn_max0(1.0f - (pl * pl) / (a.sp2 * d2));
            wz = u * u;
        }
        g = wn * wz;
    }
    const float ex = qc.x - pc.x, ey = qc.y - pc.y, ez = qc.z - pc.z;
    const float de2 = dn_dot(ex, ey, ez, ex, ey, ez);
    const float wc = 1.0f / (1.0f + (de2 * a.cl) / a.sc2);
    const float w = (h * g) * wc;
    acc.W = acc.W + w;
    acc.r = __builtin_fmaf(w, qc.x, acc.r);
    acc.g = __builtin_fmaf(w, qc.y, acc.g);
    acc.b = __builtin_fmaf(w, qc.z, acc.b);
}

__device__ __forceinline__ float dn_k(int i) { // k = {1/16, 1/4, 3/8, 1/4, 1/16}: every product k[i]·k[j] is exact in f32
    return i == 0 ? 0.375f : (i == 1 || i == -1) ? 0.25f : 0.0625f;
}

template <bool LAST> __device__ __forceinline__ void dn_store(const DenoiseArgs& a, size_t p, const DnAcc& acc) {
    const float r = acc.r / acc.W, g = acc.g / acc.W, b = acc.b / acc.W;
    if (LAST) {
        const dn4 m = a.mod[p];
        a.rgb[3 * p + 0] = r * m.x;
        a.rgb[3 * p + 1] = g * m.y;
        a.rgb[3 * p + 2] = b * m.z;
    } else {
        a.dst[p] = dn4{r, g, b, 0.0f};
    }
}

// Builds the records: guides, the modulation m and the demodulated colour e = c / m.  One thread per pixel.
__global__ __launch_bounds__(256) void denoise_pack_kernel(const float* __restrict__ rgb, const int32_t* __restrict__ index,
                                                           const float* __restrict__ normal, const float* __restrict__ point,
                                                           const float* __restrict__ albedo /* NULL: m = 1 */, dn4* __restrict__ ga,
                                                           dn4* __restrict__ gb, dn4* __restrict__ mod, dn4* __restrict__ col,
                                                           size_t n_pixels) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pixels) return;
    const bool bg = index[p] < 0;
    float mr = 1.0f, mg = 1.0f, mb = 1.0f;
    if (albedo && !bg) {
        const float lo = 0.00390625f; // 2^-8
        const float ar = albedo[3 * p], ag = albedo[3 * p + 1], ab = albedo[3 * p + 2];
        mr = ar > lo ? ar : lo;
        mg = ag > lo ? ag : lo;
        mb = ab > lo ? ab : lo;
    }
    ga[p] = dn4{normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], bg ? 1.0f : 0.0f};
    gb[p] = dn4{point[3 * p], point[3 * p + 1], point[3 * p + 2], 0.0f};
    mod[p] = dn4{mr, mg, mb, 0.0f};
    col[p] = dn4{rgb[3 * p] / mr, rgb[3 * p + 1] / mg, rgb[3 * p + 2] / mb, 0.0f};
}

// One level, taps fetched straight from global memory (the 25 taps of neighbouring pixels overlap: L1 / L2 serve them).
template <bool LAST> __global__ __launch_bounds__(256) void denoise_level_direct_kernel(const DenoiseArgs a) {
    const int x = (int)(blockIdx.x * kDnTileW + threadIdx.x % kDnTileW);
    const int y = (int)(blockIdx.y * kDnTileH + threadIdx.x / kDnTileW);
    if (x >= (int)a.width || y >= (int)a.height) return;
    const size_t p = (size_t)y * a.width + x;
    const dn4 pa = a.ga[p], pb = a.gb[p], pc = a.src[p];
    DnAcc acc{0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = -2; j <= 2; ++j) {
        const int qy = y + j * a.stride;
        if (qy < 0 || qy >= (int)a.height) continue;
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int qx = x + i * a.stride;
            if (qx < 0 || qx >= (int)a.width) continue;
            const size_t q = (size_t)qy * a.width + qx;
            dn_tap(pa, pb, pc, a.ga[q], a.gb[q], a.src[q], dn_k(i) * dn_k(j), a, acc);
        }
    }
    dn_store<LAST>(a, p, acc);
}

// One level at stride S = 2^LOG2S <= 4, the tile and a halo of 2·S pixels staged in LDS: (32 + 4S) x (8 + 4S) records of
// 3 x 16 B (20.3 / 30 / 54 KiB).  Each array is read with ds_read_b128 at consecutive 16-byte slots by consecutive lanes: the
// 16 lanes of a service group touch 16 different slots of one 256-byte bank row, so no tap read conflicts (a tap's offset i·S
// shifts all lanes alike; lanes 32..63 are on the next tile row and in other groups).
template <int LOG2S, bool LAST> __global__ __launch_bounds__(256) void denoise_level_lds_kernel(const DenoiseArgs a) {
    constexpr int S = 1 << LOG2S, H = 2 * S, TW = kDnTileW + 2 * H, TH = kDnTileH + 2 * H;
    __shared__ dn4 sa[TH * TW], sb[TH * TW], sc[TH * TW];
    const int x0 = (int)(blockIdx.x * kDnTileW) - H, y0 = (int)(blockIdx.y * kDnTileH) - H;
    for (int t = (int)threadIdx.x; t < TW * TH; t += 256) {
        const int gx = x0 + t % TW, gy = y0 + t / TW;
        dn4 va{0.0f, 0.0f, 0.0f, 0.0f}, vb = va, vc = va;
        if (gx >= 0 && gx < (int)a.width && gy >= 0 && gy < (int)a.height) { // (slots outside the frame are never used as taps)
            const size_t q = (size_t)gy * a.width + gx;
            va = a.ga[q], vb = a.gb[q], vc = a.src[q];
        }
        sa[t] = va, sb[t] = vb, sc[t] = vc;
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x % kDnTileW) + H, ly = (int)(threadIdx.x / kDnTileW) + H;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= (int)a.width || y >= (int)a.height) return;
    const int c = ly * TW + lx;
    const dn4 pa = sa[c], pb = sb[c], pc = sc[c];
    DnAcc acc{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
        const int qy = y + j * S;
        if (qy < 0 || qy >= (int)a.height) continue;
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int qx = x + i * S;
            if (qx < 0 || qx >= (int)a.width) continue;
            const int q = c + j * S * TW + i * S;
            dn_tap(pa, pb, pc, sa[q], sb[q], sc[q], dn_k(i) * dn_k(j), a, acc);
        }
    }
    dn_store<LAST>(a, (size_t)y * a.width + x, acc);
}

// ---- the variance-guided mode (rayz_hip_denoiser_run_guided) ----------------------------------------------------
// The SVGF spatial stage (Schied et al. 2017) on §4.11's guides: the colour distance of a tap is measured in units of the centre
// pixel's own variance — the caller's per-channel estimate (§4.12), demodulated, channels summed, which rides in the colour
// record's .w and is filtered along with the colour (weights squared), so each level sees the variance its input really has.
// A level reads the same three records per tap as the unguided one; the 3x3 variance prefilter reads only their .w slots.
// Everything a tap computes is in dn_tap_guided(), the prefilter's tap in dn_vtap(); both level forms call them in one order.
constexpr float kDnVarCap = 4294967296.0f; // VCAP = 2^32: "no estimate: trust the guides only"

struct DenoiseGuidedArgs {
    const dn4* __restrict__ ga;   // per pixel {n.x, n.y, n.z, bg ? 1 : 0}
    const dn4* __restrict__ gb;   // per pixel {P.x, P.y, P.z, 0}
    const dn4* __restrict__ mod;  // per pixel {m.r, m.g, m.b, 0}: read by the last level only
    const dn4* __restrict__ src;  // this level's colours and variance {e.r, e.g, e.b, v}
    dn4* __restrict__ dst;        // next level's (not the last level)
    float* __restrict__ rgb;      // packed RGB out (the last level)
    float* __restrict__ var;      // the last level's variance out, one float per pixel, or NULL
    uint32_t width, height;
    int stride;                   // 2^l
    uint32_t normal_power_log2;
    float sp2;                    // f32(sigma_plane) x f32(sigma_plane)
    float sc2;                    // f32(sigma_color) x f32(sigma_color), sigma_color in standard deviations; +inf: wc = 1 exactly
    float vf;                     // f32(var_floor)
};

struct DnAccG {
    float W, r, g, b, V;
};

__device__ __forceinline__ float dn_gk(int i) { return i == 0 ? 0.5f : 0.25f; } // gk = {1/4, 1/2, 1/4}

// One tap of the 3x3 variance prefilter: the tap's bg flag and variance (the .w slots of its ga and colour records).
__device__ __forceinline__ void dn_vtap(const bool bgp, const float qbg, const float qv, const float gg, float& G, float& A) {
    if ((qbg != 0.0f) != bgp) return;
    G = G + gg;
    A = __builtin_fmaf(gg, qv, A);
}

// One tap: as dn_tap (h, g and the skipped background-versus-hit tap are §4.11's, restated here because dn_tap keeps its own
// colour term), with wc = 1 / (1 + de2 / den), den = sc2·(gv + vf) of the CENTRE pixel, and the variance sum V.
__device__ __forceinline__ void dn_tap_guided(const dn4 pa, const dn4 pb, const dn4 pc, const dn4 qa, const dn4 qb, const dn4 qc,
                                              const float h, const float den, const DenoiseGuidedArgs& a, DnAccG& acc) {
    const bool bgp = pa.w != 0.0f, bgq = qa.w != 0.0f;
    float g = 1.0f;
    if (bgp || bgq) {
        if (!(bgp && bgq)) return;
    } else {
        float wn = dn_max0(dn_dot(pa.x, pa.y, pa.z, qa.x, qa.y, qa.z));
        for (uint32_t k = 0; k < a.normal_power_log2; ++k) wn = wn * wn;
        const float vx = qb.x - pb.x, vy = qb.y - pb.y, vz = qb.z - pb.z;
        const float d2 = dn_dot(vx, vy, vz, vx, vy, vz);
        const float pl = dn_dot(pa.x, pa.y, pa.z, vx, vy, vz);
        float wz = 1.0f;
        if (d2 != 0.0f) {
            const float u = dn_max0(1.0f - (pl * pl) / (a.sp2 * d2));
            wz = u * u;
        }
        g = wn * wz;
    }
    const float ex = qc.x - pc.x, ey = qc.y - pc.y, ez = qc.z - pc.z;
    const float de2 = dn_dot(ex, ey, ez, ex, ey, ez);
    const float wc = 1.0f / (1.0f + de2 / den);
    const float w = (h * g) * wc;
    acc.W = acc.W + w;
    acc.r = __builtin_fmaf(w, qc.x, acc.r);
    acc.g = __builtin_fmaf(w, qc.y, acc.g);
    acc.b = __builtin_fmaf(w, qc.z, acc.b);
    acc.V = __builtin_fmaf(w * w, qc.w, acc.V);
}

template <bool LAST> __device__ __forceinline__ void dn_store_guided(const DenoiseGuidedArgs& a, size_t p, const DnAccG& acc) {
    const float r = acc.r / acc.W, g = acc.g / acc.W, b = acc.b / acc.W, v = acc.V / (acc.W * acc.W);
    if (LAST) {
        const dn4 m = a.mod[p];
        a.rgb[3 * p + 0] = r * m.x;
        a.rgb[3 * p + 1] = g * m.y;
        a.rgb[3 * p + 2] = b * m.z;
        if (a.var) a.var[p] = v;
    } else {
        a.dst[p] = dn4{r, g, b, v};
    }
}

// denoise_pack_kernel plus the variance slot: v = clamp of Σ_ch var_ch / m_ch², a NaN or anything not below VCAP becoming VCAP.
__global__ __launch_bounds__(256) void dng_pack_kernel(const float* __restrict__ rgb, const float* __restrict__ var_rgb,
                                                       const int32_t* __restrict__ index, const float* __restrict__ normal,
                                                       const float* __restrict__ point, const float* __restrict__ albedo /* NULL: m = 1 */,
                                                       dn4* __restrict__ ga, dn4* __restrict__ gb, dn4* __restrict__ mod,
                                                       dn4* __restrict__ col, size_t n_pixels) {
    const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pixels) return;
    const bool bg = index[p] < 0;
    float mr = 1.0f, mg = 1.0f, mb = 1.0f;
    if (albedo && !bg) {
        const float lo = 0.00390625f; // 2^-8
        const float ar = albedo[3 * p], ag = albedo[3 * p + 1], ab = albedo[3 * p + 2];
        mr = ar > lo ? ar : lo;
        mg = ag > lo ? ag : lo;
        mb = ab > lo ? ab : lo;
    }
    const float t = ((var_rgb[3 * p] / (mr * mr)) + (var_rgb[3 * p + 1] / (mg * mg))) + (var_rgb[3 * p + 2] / (mb * mb));
    const float v = !(t < kDnVarCap) ? kDnVarCap : (t > 0.0f ? t : 0.0f);
    ga[p] = dn4{normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], bg ? 1.0f : 0.0f};
    gb[p] = dn4{point[3 * p], point[3 * p + 1], point[3 * p + 2], 0.0f};
    mod[p] = dn4{mr, mg, mb, 0.0f};
    col[p] = dn4{rgb[3 * p] / mr, rgb[3 * p + 1] / mg, rgb[3 * p + 2] / mb, v};
}

// One guided level, taps from global memory.  The 3x3 prefilter is nine more pixels at distance 1, of which only the bg flag and
// the variance are read (one dword each).
template <bool LAST> __global__ __launch_bounds__(256) void dng_level_direct_kernel(const DenoiseGuidedArgs a) {
    const int x = (int)(blockIdx.x * kDnTileW + threadIdx.x % kDnTileW);
    const int y = (int)(blockIdx.y * kDnTileH + threadIdx.x / kDnTileW);
    if (x >= (int)a.width || y >= (int)a.height) return;
    const size_t p = (size_t)y * a.width + x;
    const dn4 pa = a.ga[p], pb = a.gb[p], pc = a.src[p];
    const bool bgp = pa.w != 0.0f;
    float G = 0.0f, A = 0.0f;
#pragma unroll
    for (int j = -1; j <= 1; ++j) {
        const int qy = y + j;
        if (qy < 0 || qy >= (int)a.height) continue;
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
            const int qx = x + i;
            if (qx < 0 || qx >= (int)a.width) continue;
            const size_t q = (size_t)qy * a.width + qx;
            dn_vtap(bgp, a.ga[q].w, a.src[q].w, dn_gk(i) * dn_gk(j), G, A);
        }
    }
    const float den = a.sc2 * (A / G + a.vf);
    DnAccG acc{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    for (int j = -2; j <= 2; ++j) {
        const int qy = y + j * a.stride;
        if (qy < 0 || qy >= (int)a.height) continue;
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int qx = x + i * a.stride;
            if (qx < 0 || qx >= (int)a.width) continue;
            const size_t q = (size_t)qy * a.width + qx;
            dn_tap_guided(pa, pb, pc, a.ga[q], a.gb[q], a.src[q], dn_k(i) * dn_k(j), den, a, acc);
        }
    }
    dn_store_guided<LAST>(a, p, acc);
}

// One guided level at stride S <= 4 from LDS: denoise_level_lds_kernel's tile and halo (2·S >= 2, so the 3x3 prefilter's taps at
// distance 1 are staged too), the same slots and the same conflict-free reads.
template <int LOG2S, bool LAST> __global__ __launch_bounds__(256) void dng_level_lds_kernel(const DenoiseGuidedArgs a) {
    constexpr int S = 1 << LOG2S, H = 2 * S, TW = kDnTileW + 2 * H, TH = kDnTileH + 2 * H;
    __shared__ dn4 sa[TH * TW], sb[TH * TW], sc[TH * TW];
    const int x0 = (int)(blockIdx.x * kDnTileW) - H, y0 = (int)(blockIdx.y * kDnTileH) - H;
    for (int t = (int)threadIdx.x; t < TW * TH; t += 256) {
        const int gx = x0 + t % TW, gy = y0 + t / TW;
        dn4 va{0.0f, 0.0f, 0.0f, 0.0f}, vb = va, vc = va;
        if (gx >= 0 && gx < (int)a.width && gy >= 0 && gy < (int)a.height) { // (slots outside the frame are never used as taps)
            const size_t q = (size_t)gy * a.width + gx;
            va = a.ga[q], vb = a.gb[q], vc = a.src[q];
        }
        sa[t] = va, sb[t] = vb, sc[t] = vc;
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x % kDnTileW) + H, ly = (int)(threadIdx.x / kDnTileW) + H;
    const int x = x0 + lx, y = y0 + ly;
    if (x >= (int)a.width || y >= (int)a.height) return;
    const int c = ly * TW + lx;
    const dn4 pa = sa[c], pb = sb[c], pc = sc[c];
    const bool bgp = pa.w != 0.0f;
    float G = 0.0f, A = 0.0f;
#pragma unroll
    for (int j = -1; j <= 1; ++j) {
        const int qy = y + j;
        if (qy < 0 || qy >= (int)a.height) continue;
#pragma unroll
        for (int i = -1; i <= 1; ++i) {
            const int qx = x + i;
            if (qx < 0 || qx >= (int)a.width) continue;
            const int q = c + j * TW + i;
            dn_vtap(bgp, sa[q].w, sc[q].w, dn_gk(i) * dn_gk(j), G, A);
        }
    }
    const float den = a.sc2 * (A / G + a.vf);
    DnAccG acc{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int j = -2; j <= 2; ++j) {
        const int qy = y + j * S;
        if (qy < 0 || qy >= (int)a.height) continue;
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int qx = x + i * S;
            if (qx < 0 || qx >= (int)a.width) continue;
            const int q = c + j * S * TW + i * S;
            dn_tap_guided(pa, pb, pc, sa[q], sb[q], sc[q], dn_k(i) * dn_k(j), den, a, acc);
        }
    }
    dn_store_guided<LAST>(a, (size_t)y * a.width + x, acc);
}

// ---- host side: the launches (denoiser.hpp owns the handle, the validation and the stream) -------------------------------------
inline dim3 denoise_grid(uint32_t width, uint32_t height) {
    return dim3((width + kDnTileW - 1) / kDnTileW, (height + kDnTileH - 1) / kDnTileH);
}

inline void denoise_launch_pack(hipStream_t st, const float* rgb, const int32_t* index, const float* normal, const float* point,
                                const float* albedo, dn4* ga, dn4* gb, dn4* mod, dn4* col, size_t n_pixels) {
    hipLaunchKernelGGL(denoise_pack_kernel, dim3((uint32_t)((n_pixels + 255) / 256)), dim3(256), 0, st, rgb, index, normal, point,
                       albedo, ga, gb, mod, col, n_pixels);
}

// Level l of `a` (stride, cl set by the caller); `lds` picks the staged form, which exists for l <= kDnMaxLdsLog2 only.
template <bool LAST> inline void denoise_launch_level(hipStream_t st, const DenoiseArgs& a, uint32_t l, bool lds) {
    const dim3 grid = denoise_grid(a.width, a.height), block(256);
    if (lds && l == 0) hipLaunchKernelGGL((denoise_level_lds_kernel<0, LAST>), grid, block, 0, st, a);
    else if (lds && l == 1) hipLaunchKernelGGL((denoise_level_lds_kernel<1, LAST>), grid, block, 0, st, a);
    else if (lds && l == 2) hipLaunchKernelGGL((denoise_level_lds_kernel<2, LAST>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((denoise_level_direct_kernel<LAST>), grid, block, 0, st, a);
}

inline void denoise_launch_pack_guided(hipStream_t st, const float* rgb, const float* var_rgb, const int32_t* index, const float* normal,
                                       const float* point, const float* albedo, dn4* ga, dn4* gb, dn4* mod, dn4* col, size_t n_pixels) {
    hipLaunchKernelGGL(dng_pack_kernel, dim3((uint32_t)((n_pixels + 255) / 256)), dim3(256), 0, st, rgb, var_rgb, index, normal, point,
                       albedo, ga, gb, mod, col, n_pixels);
}

// The guided form of denoise_launch_level.
template <bool LAST> inline void denoise_launch_level_guided(hipStream_t st, const DenoiseGuidedArgs& a, uint32_t l, bool lds) {
    const dim3 grid = denoise_grid(a.width, a.height), block(256);
    if (lds && l == 0) hipLaunchKernelGGL((dng_level_lds_kernel<0, LAST>), grid, block, 0, st, a);
    else if (lds && l == 1) hipLaunchKernelGGL((dng_level_lds_kernel<1, LAST>), grid, block, 0, st, a);
    else if (lds && l == 2) hipLaunchKernelGGL((dng_level_lds_kernel<2, LAST>), grid, block, 0, st, a);
    else hipLaunchKernelGGL((dng_level_direct_kernel<LAST>), grid, block, 0, st, a);
}

} // namespace rayz_dev
