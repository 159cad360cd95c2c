// sampled_kernel.hpp — sampled G-buffers (rayz_hip_scene_query_camera_sampled): the device code.
//
// Per pixel of the shard, samples s = 0 .. n-1: the camera segment of the render's path s of that pixel — a Pcg32 seeded with
// seed_path(seed, (py·width + px)·spp + s), then camera_ray (jitter, lens, time: §4.1 / §4.2) — through `findHit` as a NEAREST
// query runs it, and the record's albedo, normal and t added to the pixel's sums in sample order; the last sample divides and
// stores the means.  Every sample is the query kernels' own scan (flat list) or walk (BVH): the same device functions in the same
// order, as chain_kernel.hpp's segments are.  Every lane of a wave runs the same n samples.
//
// A lane carries NO sums through a scan or a walk (the BVH walk sits at its register limit, chain_kernel.hpp): the seven sums and
// the hit count of pixel entry j live in eight words of R at sums[8 j] of a workspace the scene owns, read back and rewritten by
// the lane that owns the pixel — sample 0 reads nothing (the sums start at +0), the last sample writes nothing back.  And a wave
// carries none of the call's own words through them either: the output pointers, the workspace, the seed and the path ids' stride
// are read from DEVICE memory where they are used, as a chain call's output pointers are (with them among the kernel's arguments
// the f64 walk over 16-bit nodes compiled to a kernel with a scratch frame).
//
// The kernels live in a namespace of their own: rayz_dev holds exactly the kernels it held.  Included by rayz_hip.hip; the host
// side is sampled.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bvh_walk.hpp"
#include "device_math.hpp"
#include "device_types.hpp"
#include "flat_scan.hpp"
#include "path_queue.hpp"
#include "query_kernel.hpp"
#include "shade.hpp"

namespace rayz_dev_sampled {
using namespace rayz_dev;

// A sampled call's own words: where its results go (each optional), its workspace and the path ids' seed and stride.  Read from
// DEVICE memory (SampledArgs::out) where they are used; put there by chain_outputs_kernel, as a chain call's ChainStores are.
template <class R> struct SampledStores {
    R *albedo, *normal, *t;
    uint32_t* hits;
    R* sums;                 // [kSumWords · q.n], 16-byte aligned; not touched when samples == 1
    unsigned long long seed; // params->seed
    unsigned long long spp;  // params->samples_per_px: the stride of the path ids
};
constexpr size_t kSampledStoreWords = 7;
constexpr uint32_t kSumWords = 8; // of R per pixel: A.x A.y A.z N.x | N.y N.z T hits (the count in the word's low 32 bits)

template <class R> struct SampledArgs {
    QueryArgs<R> q;       // the camera form (q.rays == NULL, q.kind = nearest): scene, camera, deal, tmin, counters; its output
                          // pointers stay NULL
    const SampledStores<R>* out; // DEVICE memory
    uint32_t samples;     // n: 1 .. spp
};

// The hit count as a word of R: the inverse of bits().
template <class R> __device__ __forceinline__ R count_word(uint32_t h);
template <> __device__ __forceinline__ float count_word<float>(uint32_t h) { return __builtin_bit_cast(float, h); }
template <> __device__ __forceinline__ double count_word<double>(uint32_t h) { return __builtin_bit_cast(double, (uint64_t)h); }

// Pixel i of the shard as query_ray deals it: the entry its results go to (local row · width + column) and its GLOBAL coordinates.
template <class R> __device__ __forceinline__ uint32_t sampled_pixel(const QueryArgs<R>& A, uint32_t i, uint32_t& px, uint32_t& py) {
    uint32_t lp = i;
    if (lp < A.tiled_pixels) {
        const uint32_t tile = lp >> 6, w8 = A.width >> 3, trow = tile / w8, tcol = tile - trow * w8;
        lp = (trow * 8u + ((lp >> 3) & 7u)) * A.width + tcol * 8u + (lp & 7u);
    }
    const uint32_t lr = lp / A.width;
    px = lp - lr * A.width;
    const uint32_t tl = lr / A.tile_rows, within = lr - tl * A.tile_rows;
    py = (tl * A.shard_count + A.shard_index) * A.tile_rows + within;
    return lp;
}

// The camera segment of the render's path s of pixel (px, py).
template <class R>
__device__ __forceinline__ void sampled_ray(const SampledArgs<R>& A, uint32_t px, uint32_t py, uint32_t s, V<R>& o, V<R>& d, R& time) {
    const RAYZ_GLOBAL SampledStores<R>* P = (const RAYZ_GLOBAL SampledStores<R>*)A.out; // (fetched here: chain_step)
    asm volatile("" : "+s"(P));
    Pcg32 g;
    g.seed_path(P->seed, ((unsigned long long)py * A.q.width + px) * P->spp + s);
    camera_ray<R>(A.q.cam, g, px, py, o, d, time);
}

// What the lane of pixel entry j does with the nearest hit (tbest, ibest) of sample s on ray (o, d, time): the record as
// query_store forms it — normal facing the ray, albedo —, then one add per sum; the last sample divides and stores.
template <class R>
__device__ __forceinline__ void sampled_add(const SampledArgs<R>& A, uint32_t j, uint32_t s, V<R> o, V<R> d, R time, R tbest, int ibest) {
    typedef typename VecOf<R>::type r4;
    const QueryArgs<R>& Q = A.q;
    asm volatile("" : "+v"(j)); // (the entry's addresses are formed HERE, not in front of the sample loop: chain_step)
    V<R> nrm{0, 0, 0}, alb{R(1), R(1), R(1)}; // a miss adds 1 to the albedo's sums and nothing to the others
    if (ibest >= 0) {
        V<R> pt{0, 0, 0};
        uint32_t mat_idx;
        if ((uint32_t)ibest < Q.sc.n_spheres) {
            const r4 q = Q.sc.sph_pool[2 * ibest], w4 = Q.sc.sph_pool[2 * ibest + 1];
            sphere_hit_record<R>(q, w4, o, d, time, tbest, pt, nrm);
            mat_idx = bits(w4.w);
        } else {
            const uint32_t ti = (uint32_t)ibest - Q.sc.n_spheres;
            const r4 a = Q.sc.tri[3 * ti], b = Q.sc.tri[3 * ti + 1], e = Q.sc.tri[3 * ti + 2];
            pt = {fm(d.x, tbest, o.x), fm(d.y, tbest, o.y), fm(d.z, tbest, o.z)};
            nrm = unit(cross3(V<R>{b.x, b.y, b.z}, V<R>{e.x, e.y, e.z}));
            mat_idx = bits(a.w);
        }
        face_forward<R>(d, nrm);
        const r4 m = Q.sc.mat[mat_idx];
        alb = (bits(m.x) & 0xffu) == 2u ? V<R>{R(1), R(1), R(1)} : texture_value<R>(Q.sc.tex, bits(m.y), pt);
    }
    const RAYZ_GLOBAL SampledStores<R>* P = (const RAYZ_GLOBAL SampledStores<R>*)A.out; // (the pointers fetched here: chain_step)
    asm volatile("" : "+s"(P));
    r4* W = (r4*)(P->sums + (size_t)kSumWords * j);
    r4 lo{R(0), R(0), R(0), R(0)}, hi{R(0), R(0), R(0), R(0)};
    uint32_t hits = 0;
    if (s != 0u) {
        lo = W[0];
        hi = W[1];
        hits = bits(hi.w);
    }
    lo.x = lo.x + alb.x, lo.y = lo.y + alb.y, lo.z = lo.z + alb.z;
    if (ibest >= 0) {
        lo.w = lo.w + nrm.x, hi.x = hi.x + nrm.y, hi.y = hi.y + nrm.z;
        hi.z = hi.z + tbest;
        ++hits;
    }
    if (s + 1u != A.samples) {
        W[0] = lo;
        W[1] = r4{hi.x, hi.y, hi.z, count_word<R>(hits)};
        return;
    }
    const R n = (R)A.samples, h = (R)hits;
    if (P->albedo) P->albedo[3ull * j] = lo.x / n, P->albedo[3ull * j + 1] = lo.y / n, P->albedo[3ull * j + 2] = lo.z / n;
    if (P->normal) {
        P->normal[3ull * j] = hits ? lo.w / h : R(0);
        P->normal[3ull * j + 1] = hits ? hi.x / h : R(0);
        P->normal[3ull * j + 2] = hits ? hi.y / h : R(0);
    }
    if (P->t) P->t[j] = hits ? hi.z / h : (R)__builtin_inff();
    if (P->hits) P->hits[j] = hits;
}

// Flat list: one pixel per lane, every sample the scan of query_kernel (XZ form).  Lanes past the frame trace its last pixel's
// samples (full EXEC in the scan) and store nothing.
template <class R> __global__ __launch_bounds__(256, 4) void sampled_kernel(const SampledArgs<R> A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool valid = i < A.q.n;
    uint32_t px, py;
    const uint32_t j = sampled_pixel<R>(A.q, valid ? i : A.q.n - 1u, px, py);
    for (uint32_t s = 0; s < A.samples; ++s) {
        V<R> o, d;
        R time;
        sampled_ray<R>(A, px, py, s, o, d, time);
        ScanRay<R> ray[1];
        const V<R> ud = unit(d);
        scan_begin<R, 1>(ray[0], o, d, ud, time);
        ray[0].tbest = (R)__builtin_inff();
        scan_sphere_classes<R, 1>(A.q.sc, ray, A.q.tmin);
        narrow_flush<R, 1>(A.q.sc, ray, A.q.tmin);
        scan_triangles<R, 1>(A.q.sc, ray, A.q.tmin);
        if (valid) sampled_add<R>(A, j, s, o, d, time, ray[0].tbest, ray[0].ibest);
    }
}

// BVH: persistent workgroups, 64 pixels (one 8x8 tile) per wave at a time, every sample the walk of query_kernel_bvh.  ONE loop
// over the samples of all the wave's tiles, as chain_kernel_bvh's over its segments: a wave whose sample counter has reached n takes
// its next 64 pixels.
template <class R, bool QUANT> __global__ __launch_bounds__(RAYZ_BVH_WG, (bvh_waves<R>() * 256 >= RAYZ_BVH_WG ? bvh_waves<R>() * 256 / RAYZ_BVH_WG : 1))
void sampled_kernel_bvh(const SampledArgs<R> A) {
    typedef typename VecOf<R>::type r4;
    const QueryArgs<R>& Q = A.q;
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t n_nodes = Q.sc.bvh_n_nodes;
    const float tmin32 = round_down_f32(Q.tmin);
    extern __shared__ uint32_t lds_words[]; // (the set-up and the oversized hittables' pre-walk: query_kernel_bvh's)
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)lds_words != 0u) {
        if (threadIdx.x == 0) Q.counters[31] = 1ull;
        return;
    }
    f4* top = (f4*)lds_words;
    uint32_t* stack = lds_words + Q.bvh_top_words + kBvhWg + threadIdx.x;
    for (uint32_t k = threadIdx.x; k < Q.sc.bvh_top / 16u; k += kBvhWg) top[k] = Q.sc.bvh_nodes[k];
    const f4* nodes_base = scalar_base(Q.sc.bvh_nodes);
    stack[0] = kBvhDone;
    unsigned char* big_lds = (unsigned char*)(lds_words + Q.bvh_big_words);
    if (threadIdx.x < 2u * Q.sc.bvh_n_big_leaves) {
        const uint32_t desc = Q.sc.bvh_big[threadIdx.x >> 1], jj = threadIdx.x & 1u;
        if (jj < (desc & 3u)) {
            const uint32_t slot = (desc >> 4) + jj;
            d4* dst64 = (d4*)(big_lds + threadIdx.x * bvh_big_entry_bytes<R>());
            dst64[0] = Q.sc.bvh_sph64[2 * slot];
            dst64[1] = Q.sc.bvh_sph64[2 * slot + 1];
            r4* dst = (r4*)(dst64 + 2);
            const r4* rec = Q.sc.bvh_leaf + (size_t)Q.sc.bvh_leaf_stride * slot;
            dst[0] = rec[0];
            dst[1] = rec[1];
            dst[2] = Q.sc.bvh_leaf_stride > 2u ? rec[2] : rec[1];
        }
    }
    __syncthreads();
    uint32_t node_tests = 0, sphere_tests = 0;
#ifdef RAYZ_BVH_PROFILE // (the measurement build's box step times its node fetch: counted, not reported, as for queries)
    unsigned long long fetch_ticks = 0;
#define RAYZ_SAMPLED_FETCH , fetch_ticks
#else
#define RAYZ_SAMPLED_FETCH
#endif
    BvhQuery<R> q;
    uint32_t j = 0, px = 0, py = 0, s = A.samples;
    bool valid = false;
    for (;;) {
        if (s == A.samples) { // (wave-uniform) the wave's pixels are done, or it has none yet: the next 64
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(&Q.counters[0], 64ull);
            base = __shfl(base, 0);
            if (base >= (unsigned long long)Q.n) break;
            const uint32_t i = (uint32_t)base + lane;
            valid = i < Q.n;
            j = sampled_pixel<R>(Q, valid ? i : Q.n - 1u, px, py);
            s = 0;
        }
        {
            V<R> o, d;
            R time;
            sampled_ray<R>(A, px, py, s, o, d, time);
            const V<R> ud = unit(d);
            bvh_begin<R, QUANT>(q, Q.sc, o, d, ud, valid ? n_nodes : 0u);
            q.tbest = (R)__builtin_inff();
            q.tb32 = round_up_f32((R)__builtin_inff());
            if (Q.sc.bvh_n_big_leaves != 0u && valid) {
                for (uint32_t k = 0; k < Q.sc.bvh_n_big_leaves; ++k) {
                    const uint32_t desc = Q.sc.bvh_big[k];
                    sphere_tests += desc & 3u;
                    for (uint32_t jj = 0; jj < (desc & 3u); ++jj) {
                        const d4* rec64 = (const d4*)(big_lds + (2u * k + jj) * bvh_big_entry_bytes<R>());
                        const r4* rec = (const r4*)(rec64 + 2);
                        const r4 cc = rec[0], v = rec[1], w = rec[2];
                        if (bvh_leaf_eval<R>(Q.sc, q, desc, jj, cc, v, o, d, ud, time, Q.tmin, &w) != 0u)
                            bvh_candidate_eval<R>(q, rec64[0], rec64[1], (int)bits(v.w), o, d, time, Q.tmin);
                    }
                }
            }
            for (;;) {
                if constexpr (sizeof(R) == 8) q.tb32 = round_up_f32(q.tbest);
                bool can_step = q.cur < kBvhDone;
                int n_can = __popcll(__ballot(can_step));
                bool run = n_can != 0 && (n_can >= kBvhKeepStepping || __ballot((int32_t)q.cur < 0) == 0ull);
                while (run) {
                    if (can_step) bvh_node_step<R, kBvhWg, QUANT>(Q.sc, nodes_base, q, tmin32, stack RAYZ_SAMPLED_FETCH);
                    {
                        const bool again = q.cur < kBvhDone;
                        node_tests += 2u * (uint32_t)__popcll(__ballot(again));
                        if (again) bvh_node_step<R, kBvhWg, QUANT>(Q.sc, nodes_base, q, tmin32, stack RAYZ_SAMPLED_FETCH);
                    }
                    node_tests += 2u * (uint32_t)n_can;
                    can_step = q.cur < kBvhDone;
                    n_can = __popcll(__ballot(can_step));
                    run = n_can != 0 && (n_can >= kBvhKeepStepping || __ballot((int32_t)q.cur < 0) == 0ull);
                }
                const bool parked = (int32_t)q.cur < 0;
                if (__ballot(parked) == 0ull) break;
                uint32_t cand0 = 0, cand1 = 0;
                int pool0 = 0, pool1 = 0;
                if (parked) {
                    const uint32_t leaf = q.cur & ~kBvhLeafFlag;
                    sphere_tests += leaf & 3u;
                    bvh_pop<R, kBvhWg>(q, stack);
                    bvh_leaf_pair<R>(Q.sc, q, leaf, o, d, ud, time, Q.tmin, cand0, cand1, pool0, pool1);
                }
                if (__ballot((cand0 | cand1) != 0u) != 0ull) bvh_candidate_passes<R>(Q.sc, q, cand0, cand1, pool0, pool1, o, d, time, Q.tmin);
                if (__ballot(q.cur != kBvhDone) == 0ull) break;
            }
            if (valid) sampled_add<R>(A, j, s, o, d, time, q.tbest, q.ibest);
            ++s;
        }
    }
    unsigned long long t2 = sphere_tests;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t2 += __shfl_xor(t2, off);
    if (lane == 0) {
        atomicAdd(&Q.counters[2], (unsigned long long)node_tests);
        atomicAdd(&Q.counters[3], t2);
    }
}
#undef RAYZ_SAMPLED_FETCH

} // namespace rayz_dev_sampled
