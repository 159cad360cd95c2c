// adaptive.hpp — adaptive passes (include/rayz_hip.h: rayz_hip_progressive_set_adaptive, _adaptive_step,
// _run_adaptive, rayz_hip_adaptive_kat): trace only the pixels the noise estimate has not called done.
//
// An adaptive handle keeps frozen_at[i] per shard pixel (0: active; else the chunk count at which the pixel froze) and the ACTIVE
// LIST: the row-major local indices of the active pixels, in the order pixels are dealt (place_item: 8x8 tiles of the first
// tiled_pixels, then row by row), so that the 64 items a wave grabs stay neighbours however thin the list gets.  A pass
//   1. traces the window's chunks of the listed pixels (the kAdaptive trace kernels: chunk sum of entry k · n_active + j at that
//      COMPACT index — workspace and fold traffic shrink with the list),
//   2. adaptive_fold_kernel: folds them into acc and Q of those pixels (accumulate_moments_kernel's arithmetic, chunk order),
//      evaluates §4.12 at the pass's end, freezes, writes the pixel's preview and counts the block's survivors,
//   3. adaptive_scan_kernel + adaptive_scatter_kernel: the ORDERED compaction of the list into the next pass's list.
// Nothing but n_active (4 bytes, for the next launch's size) goes back to the host.
//
// THE PREVIEW RULE.  A pass writes the preview of the pixels it traced; a pixel's last write is the one of the pass it froze in,
// acc · (1 / starts[frozen_at]), which is its final value.  So a buffer that is passed to EVERY pass holds the whole frame after
// each of them.  A pass given a buffer other than the one the previous pass wrote (the first pass, and the pass after one that
// got no buffer and so wrote none: any buffer) writes ALL pixels (adaptive_frame_kernel), and so does a step on a finished run,
// which traces nothing: that is how a caller asks for the frame in a buffer of its choice.  Buffers are told apart by address.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>

#include "device_types.hpp"
#include "noise.hpp"

namespace rayz_dev {

// The initial list: entry i = the row-major local pixel dealt i-th (place_item's tile arithmetic; width % 8 == 0 wherever
// tiled_pixels != 0).
__global__ __launch_bounds__(256) void adaptive_list_init_kernel(uint32_t* __restrict__ list, uint32_t shard_pixels, uint32_t tiled_pixels,
                                                                 uint32_t width) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= shard_pixels) return;
    uint32_t lp = i;
    if (i < tiled_pixels) {
        const uint32_t tile = i >> 6, w8 = width >> 3, trow = tile / w8, tcol = tile - trow * w8;
        lp = (trow * 8u + ((i >> 3) & 7u)) * width + tcol * 8u + (i & 7u);
    }
    list[i] = lp;
}

// ---- fold, evaluate, freeze: one thread per ACTIVE entry ---------------------------------------------------------------------
// `partial`: the pass's compact chunk sums, chunk k of entry j at k · n_active + j (`chunks` may be 0: a render whose passes
// trace nothing, max_bounces = 0, still evaluates and freezes).  `sizes` = starts + c0 as in accumulate_moments_kernel;
// chunks_end = c1, samples_end = starts[c1].  acc and Q always start from memory (+0 before the first pass: the handle clears
// them), which is the first pass's "from +0".  The pixel freezes iff chunks_end >= min_chunks and rel2 <= tau2 (a NaN compares
// false).  survivors[block] = entries of this block still active afterwards, for the compaction.
template <class R>
__global__ __launch_bounds__(256) void adaptive_fold_kernel(const typename VecOf<R>::type* __restrict__ partial,
                                                            const uint32_t* __restrict__ list, uint32_t n_active,
                                                            typename VecOf<R>::type* __restrict__ acc, d4* __restrict__ q,
                                                            uint32_t* __restrict__ frozen_at, R* __restrict__ out,
                                                            const uint32_t* __restrict__ sizes, uint32_t chunks, uint32_t chunks_end,
                                                            uint32_t samples_end, uint32_t min_chunks, double floor2, double tau2,
                                                            uint32_t* __restrict__ survivors) {
    typedef typename VecOf<R>::type r4;
    __shared__ uint32_t s_cnt[4];
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    bool survives = false;
    if (j < n_active) { // (no early return: every lane takes part in the count below)
        const uint32_t lp = list[j];
        const r4 a = acc[lp];
        const d4 m = q[lp];
        R x = a.x, y = a.y, z = a.z;
        double qx = m.x, qy = m.y, qz = m.z;
        for (uint32_t k = 0; k < chunks; ++k) {
            const r4 p = partial[(size_t)k * n_active + j];
            const double n = (double)(sizes[k + 1] - sizes[k]);
            x = x + p.x;
            y = y + p.y;
            z = z + p.z;
            nz_fold<R>(qx, p.x, n);
            nz_fold<R>(qy, p.y, n);
            nz_fold<R>(qz, p.z, n);
        }
        acc[lp] = r4{x, y, z, R(0)};
        q[lp] = d4{qx, qy, qz, 0.0};
        const NzEval e = nz_eval((double)x, (double)y, (double)z, qx, qy, qz, (double)chunks_end, (double)samples_end, floor2);
        const bool freeze = chunks_end >= min_chunks && e.rel2 <= tau2;
        if (freeze) frozen_at[lp] = chunks_end;
        survives = !freeze;
        if (out) {
            const R inv = R(1) / (R)samples_end;
            out[3 * (size_t)lp + 0] = x * inv;
            out[3 * (size_t)lp + 1] = y * inv;
            out[3 * (size_t)lp + 2] = z * inv;
        }
    }
    const uint32_t cnt = (uint32_t)__popcll(__ballot(survives));
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) survivors[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

// ---- the ordered compaction ---------------------------------------------------------------------------------------------------
// One workgroup turns survivors[0 .. n_blocks) into its exclusive prefix sums in place, 1,024 counts per round with a running
// carry, and leaves the total in *n_active_out (a 1080p shard: 8 rounds).
__global__ __launch_bounds__(1024) void adaptive_scan_kernel(uint32_t* __restrict__ survivors, uint32_t n_blocks, uint32_t* __restrict__ n_active_out) {
    __shared__ uint32_t s_wave[16];
    __shared__ uint32_t s_carry;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) s_carry = 0u;
    __syncthreads();
    for (uint32_t base = 0; base < n_blocks; base += 1024u) { // (workgroup-uniform trip count)
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < n_blocks ? survivors[i] : 0u;
        uint32_t incl = v; // inclusive scan over the wave
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(incl, off);
            if (lane >= (uint32_t)off) incl += o;
        }
        if (lane == 63u) s_wave[wave] = incl;
        __syncthreads();
        uint32_t before = s_carry;
        for (uint32_t w = 0; w < wave; ++w) before += s_wave[w];
        if (i < n_blocks) survivors[i] = before + incl - v;
        __syncthreads(); // (everyone has read s_carry and s_wave)
        if (threadIdx.x == 1023u) s_carry = before + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_active_out = s_carry;
}

// Entry j of the old list survives iff its pixel is still active; it goes to offsets[block] + its rank among the block's
// survivors (lanes by ballot, waves in wave order): the old order is kept.
__global__ __launch_bounds__(256) void adaptive_scatter_kernel(const uint32_t* __restrict__ list, uint32_t n_active,
                                                               const uint32_t* __restrict__ frozen_at,
                                                               const uint32_t* __restrict__ offsets, uint32_t* __restrict__ next) {
    __shared__ uint32_t s_cnt[4];
    const uint32_t j = blockIdx.x * 256 + threadIdx.x;
    uint32_t lp = 0;
    bool survives = false;
    if (j < n_active) {
        lp = list[j];
        survives = frozen_at[lp] == 0u;
    }
    const unsigned long long mask = __ballot(survives);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_cnt[wave] = (uint32_t)__popcll(mask);
    __syncthreads();
    uint32_t at = offsets[blockIdx.x] + rank;
    for (uint32_t w = 0; w < wave; ++w) at += s_cnt[w];
    if (survives) next[at] = lp; // (at < the scan's total <= n_active: the capacity of `next`)
}

// ---- the whole frame, and the samples behind every pixel: one thread per pixel -----------------------------------------------
// N_i = starts[frozen_at[i]] for a frozen pixel, starts[chunks_done] for an active one; value = acc · (1 / N_i), the
// reciprocal-and-multiply of accumulate_kernel's preview (and what adaptive_fold_kernel wrote when the pixel froze).
template <class R>
__global__ __launch_bounds__(256) void adaptive_frame_kernel(const typename VecOf<R>::type* __restrict__ acc,
                                                             const uint32_t* __restrict__ frozen_at, const uint32_t* __restrict__ starts,
                                                             uint32_t chunks_done, R* __restrict__ out, uint32_t shard_pixels) {
    typedef typename VecOf<R>::type r4;
    const uint32_t lp = blockIdx.x * 256 + threadIdx.x;
    if (lp >= shard_pixels) return;
    const uint32_t f = frozen_at[lp];
    const R inv = R(1) / (R)starts[f ? f : chunks_done];
    const r4 a = acc[lp];
    out[3 * (size_t)lp + 0] = a.x * inv;
    out[3 * (size_t)lp + 1] = a.y * inv;
    out[3 * (size_t)lp + 2] = a.z * inv;
}

__global__ __launch_bounds__(256) void adaptive_counts_kernel(const uint32_t* __restrict__ frozen_at, const uint32_t* __restrict__ starts,
                                                              uint32_t chunks_done, uint32_t* __restrict__ counts, uint32_t shard_pixels) {
    const uint32_t lp = blockIdx.x * 256 + threadIdx.x;
    if (lp >= shard_pixels) return;
    const uint32_t f = frozen_at[lp];
    counts[lp] = starts[f ? f : chunks_done];
}

} // namespace rayz_dev
