// denoise.hpp — the G-buffer-guided à-trous denoiser's device code (its variance-guided mode §4.13;
// include/rayz_hip.h: rayz_hip_denoiser_*).
//
// An image-space filter on whole f32 frames: a PACK pass turns the caller's radiance and camera-query G-buffer into 16-byte
// aligned per-pixel records once (the guides do not change between levels), then ONE launch per level reads a colour buffer
// and writes the other, 25 taps at stride 2^l; the last level multiplies the albedo back in and writes packed RGB.
//
// The variance-guided mode is the SVGF spatial stage (Schied et al. 2017) on the same guides: the colour distance of a tap is
// measured in units of the centre pixel's own variance — the caller's per-channel estimate (§4.12), demodulated, channels summed,
// which rides in the colour record's .w and is filtered along with the colour (weights squared), so each level sees the variance
// its input really has.  A level reads the same three records per tap in either mode; the guided mode's 3x3 variance prefilter
// reads only their .w slots.  The mode is the template flag GUIDED of every kernel: one pack pass, one level body.
//
// The arithmetic is a contract (§4.11, §4.13): + - x, the FMAs written below, correctly rounded divides, comparisons — nothing
// else, so that tests/denoise_mirror.cpp and tests/denoise_guided_mirror.cpp restate it bit for bit.  Everything a tap computes is
// in dn_tap() — what the guides give it first, the same in both modes, then the mode's colour term —, the prefilter's tap in
// dn_vtap(); dn_filter_pixel() visits the taps in one order (j outer, i inner, ascending) whichever form fetches them, so the
// staging a level uses never changes a value.
//
// The guides are whatever G-buffer the caller hands in.  A camera query's are FIRST-HIT guides: a mirror or a glass ball is filtered
// by its own surface's normal and point, and the reflection in it is smoothed as if it were a texture of the ball.  A chain
// G-buffer's (rayz_hip_scene_query_camera_chain, §4.18) are those of what is SEEN in the ball; its surface KEYS
// (rayz_hip_denoiser_set_keys) ride in the gb record's .w slot as raw bits, and a tap whose key differs from the centre pixel's
// is skipped before anything else — "the ground" and "the ground seen in the ball" never mix.  Without keys the slot holds 0
// everywhere and the rule never fires.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

namespace rayz_dev {

typedef float dn4 __attribute__((ext_vector_type(4)));

constexpr int kDnTileW = 32, kDnTileH = 8;  // output pixels of a workgroup: 256 threads, a wave covers two tile rows
constexpr int kDnMaxLdsLog2 = 2;            // the LDS form exists for strides 1, 2, 4 (halo 2·s on every side)
constexpr int kDnLdsMaxStride = 2;          // levels up to this stride use it, wider ones read global memory: measured, DESIGN.md §6
                                            // (RAYZ_DEBUG_DENOISE_LDS_STRIDE overrides it for measurement)
constexpr float kDnVarCap = 4294967296.0f;  // VCAP = 2^32: "no estimate: trust the guides only"

// One level's arguments, of either mode: the plain mode leaves var and vf unused, the guided mode cl.
struct DenoiseArgs {
    const dn4* __restrict__ ga;   // per pixel {n.x, n.y, n.z, bg ? 1 : 0}
    const dn4* __restrict__ gb;   // per pixel {P.x, P.y, P.z, the surface key's 32 bits (0 without keys)}
    const dn4* __restrict__ mod;  // per pixel {m.r, m.g, m.b, 0}: read by the last level only
    const dn4* __restrict__ src;  // this level's colours {e.r, e.g, e.b, guided: the variance v, plain: 0}
    dn4* __restrict__ dst;        // next level's colours (not the last level)
    float* __restrict__ rgb;      // packed RGB out (the last level)
    float* __restrict__ var;      // guided: the last level's variance out, one float per pixel, or NULL
    float* tap;                   // packed RGB out of THIS level, re-modulated as the last level's is, or NULL (all levels but the
                                  // tapped one: rayz_hip_denoiser_run_guided_tap); never rgb
    uint32_t width, height;
    int stride;                   // 2^l
    uint32_t normal_power_log2;
    float sp2;                    // f32(sigma_plane) x f32(sigma_plane)
    float sc2;                    // f32(sigma_color) x f32(sigma_color); +inf switches the colour term off exactly (guided:
                                  // sigma_color in standard deviations)
    float cl;                     // plain: 4^l
    float vf;                     // guided: f32(var_floor)
};

__device__ __forceinline__ float dn_dot(float ax, float ay, float az, float bx, float by, float bz) {
    return __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx)); // fma(z, z', fma(y, y', x·x')): the order §4.11 states
}
__device__ __forceinline__ float dn_max0(float x) { return x > 0.0f ? x : 0.0f; } // (a NaN gives 0)

// §4.13's clamp of a variance: a NaN or anything not below VCAP becomes VCAP, anything not above 0 becomes 0.
__device__ __forceinline__ float dn_clamp_var(float t) { return !(t < kDnVarCap) ? kDnVarCap : (t > 0.0f ? t : 0.0f); }

// The surface key of a gb record: its .w slot's bits, compared as an integer (never as a float: a key is an arbitrary pattern).
// (through a float of its own: __builtin_bit_cast on the vector's element `b.w` itself reads the vector's first four bytes, b.x)
__device__ __forceinline__ uint32_t dn_key(const dn4 b) {
    const float w = b.w;
    return __builtin_bit_cast(uint32_t, w);
}

struct DnAcc {
    float W, r, g, b, V; // (V: the guided mode's variance sum)
};

struct DnTap { // the three records of a pixel
    dn4 a, b, c;
};

// The guide half of a tap, which every filter that weighs a pixel q by the guides of a pixel p shares (the à-trous levels below, the
// upscaler's taps in upscale.hpp): the records' {n, bg} and {P, ·} of the centre (pa, pb) and of the tap (qa, qb).  false: the tap is
// skipped; true: g = 1 between two background pixels, else wn·wz.
__device__ __forceinline__ bool dn_guide(const dn4 pa, const dn4 pb, const dn4 qa, const dn4 qb, const uint32_t normal_power_log2,
                                         const float sp2, float& g) {
    const bool bgp = pa.w != 0.0f, bgq = qa.w != 0.0f;
    g = 1.0f;
    if (bgp || bgq) {
        if (!(bgp && bgq)) return false; // background never mixes with a hit: the tap is skipped, as one outside the frame is
    } else {
        float wn = dn_max0(dn_dot(pa.x, pa.y, pa.z, qa.x, qa.y, qa.z));
        for (uint32_t k = 0; k < normal_power_log2; ++k) wn = wn * wn;
        const float vx = qb.x - pb.x, vy = qb.y - pb.y, vz = qb.z - pb.z;
        const float d2 = dn_dot(vx, vy, vz, vx, vy, vz);
        const float pl = dn_dot(pa.x, pa.y, pa.z, vx, vy, vz);
        float wz = 1.0f;
        if (d2 != 0.0f) {
            const float u = dn_max0(1.0f - (pl * pl) / (sp2 * d2));
            wz = u * u;
        }
        g = wn * wz;
    }
    return true;
}

// One tap: centre pixel (pa, pb, pc), tap pixel (qa, qb, qc), h = k[i]·k[j].  A tap of another surface key is skipped (§4.18); then
// the guides either skip the tap or give it g = wn·wz;
// the colour weight is wc = 1 / (1 + de2·cl / sc2), or in the guided mode 1 / (1 + de2 / den) with den = sc2·(gv + vf) of the
// CENTRE pixel, which also sums the variance V.
template <bool GUIDED>
__device__ __forceinline__ void dn_tap(const dn4 pa, const dn4 pb, const dn4 pc, const dn4 qa, const dn4 qb, const dn4 qc, const float h,
                                       const float den, const DenoiseArgs& a, DnAcc& acc) {
    if (dn_key(pb) != dn_key(qb)) return;
    float g;
    if (!dn_guide(pa, pb, qa, qb, a.normal_power_log2, a.sp2, g)) return;
    const float ex = qc.x - pc.x, ey = qc.y - pc.y, ez = qc.z - pc.z;
    const float de2 = dn_dot(ex, ey, ez, ex, ey, ez);
    const float wc = GUIDED ? 1.0f / (1.0f + de2 / den) : 1.0f / (1.0f + (de2 * a.cl) / a.sc2);
    const float w = (h * g) * wc;
    acc.W = acc.W + w;
    acc.r = __builtin_fmaf(w, qc.x, acc.r);
    acc.g = __builtin_fmaf(w, qc.y, acc.g);
    acc.b = __builtin_fmaf(w, qc.z, acc.b);
    if (GUIDED) acc.V = __builtin_fmaf(w * w, qc.w, acc.V);
}

__device__ __forceinline__ float dn_k(int i) { // k = {1/16, 1/4, 3/8, 1/4, 1/16}: every product k[i]·k[j] is exact in f32
    return i == 0 ? 0.375f : (i == 1 || i == -1) ? 0.25f : 0.0625f;
}
__device__ __forceinline__ float dn_gk(int i) { return i == 0 ? 0.5f : 0.25f; } // gk = {1/4, 1/2, 1/4}

// One tap of the guided mode's 3x3 variance prefilter: the tap's surface key, bg flag and variance (the .w slots of its three
// records); kp is the centre pixel's key.
__device__ __forceinline__ void dn_vtap(const uint32_t kp, const bool bgp, const uint32_t qk, const float qbg, const float qv, const float gg,
                                        float& G, float& A) {
    if (qk != kp) return;
    if ((qbg != 0.0f) != bgp) return;
    G = G + gg;
    A = __builtin_fmaf(gg, qv, A);
}

template <bool GUIDED, bool LAST> __device__ __forceinline__ void dn_store(const DenoiseArgs& a, size_t p, const DnAcc& acc) {
    const float r = acc.r / acc.W, g = acc.g / acc.W, b = acc.b / acc.W, v = GUIDED ? acc.V / (acc.W * acc.W) : 0.0f;
    if (LAST) {
        const dn4 m = a.mod[p];
        a.rgb[3 * p + 0] = r * m.x;
        a.rgb[3 * p + 1] = g * m.y;
        a.rgb[3 * p + 2] = b * m.z;
        if (GUIDED && a.var) a.var[p] = v;
        if (a.tap) a.tap[3 * p + 0] = r * m.x, a.tap[3 * p + 1] = g * m.y, a.tap[3 * p + 2] = b * m.z;
    } else {
        a.dst[p] = dn4{r, g, b, v};
        if (a.tap) { // the tapped level: what a run of this many levels writes as its output
            const dn4 m = a.mod[p];
            a.tap[3 * p + 0] = r * m.x, a.tap[3 * p + 1] = g * m.y, a.tap[3 * p + 2] = b * m.z;
        }
    }
}

// Builds the records: guides, the modulation m and the demodulated colour e = c / m; in the guided mode also the variance slot,
// v = the clamp of Σ_ch var_ch / m_ch² (var_rgb is not read otherwise); the surface key's bits, if there are keys.  One thread per pixel.
template <bool GUIDED>
__global__ __launch_bounds__(256) void denoise_pack_kernel(const float* __restrict__ rgb, const float* __restrict__ var_rgb,
                                                           const int32_t* __restrict__ index, const float* __restrict__ normal,
                                                           const float* __restrict__ point, const float* __restrict__ albedo /* NULL: m = 1 */,
                                                           const uint32_t* __restrict__ keys /* NULL: no keys */, dn4* __restrict__ ga, dn4* __restrict__ gb, dn4* __restrict__ mod,
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
    float v = 0.0f;
    if (GUIDED) v = dn_clamp_var(((var_rgb[3 * p] / (mr * mr)) + (var_rgb[3 * p + 1] / (mg * mg))) + (var_rgb[3 * p + 2] / (mb * mb)));
    ga[p] = dn4{normal[3 * p], normal[3 * p + 1], normal[3 * p + 2], bg ? 1.0f : 0.0f};
    gb[p] = dn4{point[3 * p], point[3 * p + 1], point[3 * p + 2], keys ? __builtin_bit_cast(float, keys[p]) : 0.0f};
    mod[p] = dn4{mr, mg, mb, 0.0f};
    col[p] = dn4{rgb[3 * p] / mr, rgb[3 * p + 1] / mg, rgb[3 * p + 2] / mb, v};
}

// Where a level fetches its taps from.  A tap source yields the records of frame pixel (qx, qy), which lies (dx, dy) from the
// thread's own; it names the level's stride, and says how far the loop over the tap rows is unrolled.
// .. straight from global memory (the 25 taps of neighbouring pixels overlap: L1 / L2 serve them), at the level's runtime stride,
// the rows not unrolled:
struct DnGlobalTaps {
    static constexpr int kRowUnroll = 1;
    const DenoiseArgs& a;
    __device__ __forceinline__ int stride() const { return a.stride; }
    __device__ __forceinline__ DnTap at(int qx, int qy, int, int) const {
        const size_t q = (size_t)qy * a.width + qx;
        DnTap t{a.ga[q], a.gb[q], a.src[q]};
        // the three loads of a tap are issued TOGETHER: left to itself the compiler fetches the record the first rule reads (the key's),
        // waits, and only then fetches the other two behind the branch — two dependent memory round trips per tap
        asm volatile("" : "+v"(t.a), "+v"(t.b), "+v"(t.c));
        return t;
    }
};
// .. from the tile staged in LDS, TW records wide, the thread's own at slot c, at the compile-time stride S, every tap unrolled:
template <int S, int TW> struct DnLdsTaps {
    static constexpr int kRowUnroll = 5;
    const dn4 *sa, *sb, *sc;
    int c;
    __device__ __forceinline__ constexpr int stride() const { return S; }
    __device__ __forceinline__ DnTap at(int, int, int dx, int dy) const {
        const int q = c + dy * TW + dx;
        DnTap t{sa[q], sb[q], sc[q]};
        asm("" : "+v"(t.b)); // (the gb record whole, one ds_read_b128, also where only its key is used: the prefilter's taps)
        return t;
    }
};

// The sums of one output pixel (x, y) of a level: the guided mode's 3x3 variance prefilter (nine pixels at distance 1, of which only
// the bg flag and the variance are used), then the 25 taps.  A tap outside the frame is skipped.  (The kernels store the result:
// with dn_store() in here the direct form costs two more vector registers.)
template <bool GUIDED, class Taps>
__device__ __forceinline__ DnAcc dn_filter_pixel(const DenoiseArgs& a, const int x, const int y, const Taps& taps) {
    const DnTap p = taps.at(x, y, 0, 0);
    float den = 0.0f;
    if (GUIDED) {
        const bool bgp = p.a.w != 0.0f;
        float G = 0.0f, A = 0.0f;
#pragma unroll
        for (int j = -1; j <= 1; ++j) {
            const int qy = y + j;
            if (qy < 0 || qy >= (int)a.height) continue;
#pragma unroll
            for (int i = -1; i <= 1; ++i) {
                const int qx = x + i;
                if (qx < 0 || qx >= (int)a.width) continue;
                const DnTap q = taps.at(qx, qy, i, j);
                dn_vtap(dn_key(p.b), bgp, dn_key(q.b), q.a.w, q.c.w, dn_gk(i) * dn_gk(j), G, A);
            }
        }
        den = a.sc2 * (A / G + a.vf);
    }
    const int s = taps.stride();
    DnAcc acc{0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll Taps::kRowUnroll
    for (int j = -2; j <= 2; ++j) {
        const int qy = y + j * s;
        if (qy < 0 || qy >= (int)a.height) continue;
#pragma unroll
        for (int i = -2; i <= 2; ++i) {
            const int qx = x + i * s;
            if (qx < 0 || qx >= (int)a.width) continue;
            const DnTap q = taps.at(qx, qy, i * s, j * s);
            dn_tap<GUIDED>(p.a, p.b, p.c, q.a, q.b, q.c, dn_k(i) * dn_k(j), den, a, acc);
        }
    }
    return acc;
}

// One level, taps fetched straight from global memory.
template <bool GUIDED, bool LAST> __global__ __launch_bounds__(256) void denoise_level_direct_kernel(const DenoiseArgs a) {
    const int x = (int)(blockIdx.x * kDnTileW + threadIdx.x % kDnTileW);
    const int y = (int)(blockIdx.y * kDnTileH + threadIdx.x / kDnTileW);
    if (x >= (int)a.width || y >= (int)a.height) return;
    const size_t p = (size_t)y * a.width + x;
    dn_store<GUIDED, LAST>(a, p, dn_filter_pixel<GUIDED>(a, x, y, DnGlobalTaps{a}));
}

// One level at stride S = 2^LOG2S <= 4, the tile and a halo of 2·S pixels staged in LDS: (32 + 4S) x (8 + 4S) records of
// 3 x 16 B (20.3 / 30 / 54 KiB); 2·S >= 2, so the prefilter's taps at distance 1 are staged too.  Each array is read with
// ds_read_b128 at consecutive 16-byte slots by consecutive lanes: the 16 lanes of a service group touch 16 different slots of one
// 256-byte bank row, so no tap read conflicts (a tap's offset i·S shifts all lanes alike; lanes 32..63 are on the next tile row and
// in other groups).
template <bool GUIDED, int LOG2S, bool LAST> __global__ __launch_bounds__(256) void denoise_level_lds_kernel(const DenoiseArgs a) {
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
    dn_store<GUIDED, LAST>(a, (size_t)y * a.width + x, dn_filter_pixel<GUIDED>(a, x, y, DnLdsTaps<S, TW>{sa, sb, sc, ly * TW + lx}));
}

// ---- host side: the launches (denoiser.hpp owns the handle, the validation and the stream) -------------------------------------
inline dim3 denoise_grid(uint32_t width, uint32_t height) {
    return dim3((width + kDnTileW - 1) / kDnTileW, (height + kDnTileH - 1) / kDnTileH);
}

inline void denoise_launch_pack(hipStream_t st, bool guided, const float* rgb, const float* var_rgb /* guided only */, const int32_t* index,
                                const float* normal, const float* point, const float* albedo, const uint32_t* keys, dn4* ga, dn4* gb, dn4* mod,
                                dn4* col, size_t n_pixels) {
    hipLaunchKernelGGL(guided ? denoise_pack_kernel<true> : denoise_pack_kernel<false>, dim3((uint32_t)((n_pixels + 255) / 256)), dim3(256), 0,
                       st, rgb, var_rgb, index, normal, point, albedo, keys, ga, gb, mod, col, n_pixels);
}

typedef void (*DnLevelKernel)(DenoiseArgs);
template <bool GUIDED, bool LAST> inline DnLevelKernel denoise_level_kernel(uint32_t l, bool lds) {
    if (lds && l == 0) return denoise_level_lds_kernel<GUIDED, 0, LAST>;
    if (lds && l == 1) return denoise_level_lds_kernel<GUIDED, 1, LAST>;
    if (lds && l == 2) return denoise_level_lds_kernel<GUIDED, 2, LAST>;
    return denoise_level_direct_kernel<GUIDED, LAST>;
}

// Level l of `a` (stride, cl set by the caller); `lds` picks the staged form, which exists for l <= kDnMaxLdsLog2 only.
inline void denoise_launch_level(hipStream_t st, bool guided, bool last, const DenoiseArgs& a, uint32_t l, bool lds) {
    const DnLevelKernel k = guided ? (last ? denoise_level_kernel<true, true>(l, lds) : denoise_level_kernel<true, false>(l, lds))
                                   : (last ? denoise_level_kernel<false, true>(l, lds) : denoise_level_kernel<false, false>(l, lds));
    hipLaunchKernelGGL(k, denoise_grid(a.width, a.height), dim3(256), 0, st, a);
}

} // namespace rayz_dev
