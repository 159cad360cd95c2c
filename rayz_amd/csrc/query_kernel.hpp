// query_kernel.hpp — ray queries on device scenes (rayz_hip_scene_query*): the argument block, the ray and the
// stores of one query, the flat-list, BVH and bounds kernels, and query_key.  The host side is query.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/rayz_hip.h"
#include "bvh_walk.hpp"
#include "device_math.hpp"
#include "device_types.hpp"
#include "flat_scan.hpp"
#include "path_queue.hpp"
#include "shade.hpp"

namespace rayz_dev {

// ---- ray queries: `findHit` on caller rays (rayz_hip_scene_query*) -------------------------------------------------
// The reference's other interface, `BVH.findHit(hittables, ray, tmin, tmax) -> ?Hit` (src/hit.zig:181-217, src/geom.zig:33-66),
// on a batch of rays: the render's own scan / walk, narrow phase and hit record, with two differences only.
// A query starts at tbest = tmax, ibest = -1 instead of +inf: with accept_root's rule (t < tbest, or t == tbest and a larger
// index than -1) that accepts exactly the roots in [tmin, tmax], the reference's inclusive `t <= maxt`.  And ANY stops a lane's
// walk at its first accepted root.  The rays are one per lane; no RNG, no shading.
constexpr uint32_t kQueryNearest = 0u, kQueryAny = 1u;
template <class R> struct QueryArgs {
    DevScene<R> sc;
    DevCamera<R> cam;
    const R* rays;            // [n · 8] {ox, oy, oz, time, dx, dy, dz, tmax}; NULL: the camera form (camera_ray_no_rng per pixel)
    R tmin;
    uint32_t n, kind;         // rays (camera form: the shard's pixels), kQueryNearest / kQueryAny
    uint32_t width, tile_rows, shard_index, shard_count, tiled_pixels; // camera form: the pixels, dealt as the render deals them
    unsigned long long* counters; // [0] batch head, [2] node tests, [3] sphere tests (BVH)
    // outputs, each optional (NULL: not written); entry i belongs to ray i (camera form: to local pixel row · width + column)
    int32_t* index;  // hittable (spheres, then triangles) or -1
    R* t;            // +inf on a miss
    R* point;        // [3 n]
    R* normal;       // [3 n] facing the ray (Hit.init)
    uint8_t* front;  // front_face
    int32_t* material;
    R* albedo;       // [3 n] texture_value at the point; (1, 1, 1) for a dielectric
    uint8_t* hit;    // ANY: 1 if some root lies in [tmin, tmax]
    uint32_t bvh_top_words, bvh_big_words; // BVH: as TraceArgs
};

// Ray i of a batch.  The camera form deals the shard's pixels in 8x8 tiles of local rows (place_item's rule) and returns where
// the pixel's results go.
template <class R>
__device__ __forceinline__ uint32_t query_ray(const QueryArgs<R>& A, uint32_t i, V<R>& o, V<R>& d, R& time, R& tmax) {
    if (A.rays) {
        const R* r = A.rays + 8ull * i;
        o = {r[0], r[1], r[2]};
        time = r[3];
        d = {r[4], r[5], r[6]};
        tmax = r[7];
        return i;
    }
    uint32_t lp = i;
    if (lp < A.tiled_pixels) {
        const uint32_t tile = lp >> 6, w8 = A.width >> 3, trow = tile / w8, tcol = tile - trow * w8;
        lp = (trow * 8u + ((lp >> 3) & 7u)) * A.width + tcol * 8u + (lp & 7u);
    }
    const uint32_t lr = lp / A.width, px = lp - lr * A.width;
    const uint32_t tl = lr / A.tile_rows, within = lr - tl * A.tile_rows;
    const uint32_t py = (tl * A.shard_count + A.shard_index) * A.tile_rows + within;
    camera_ray_no_rng<R>(A.cam, px, py, o, d, time);
    tmax = (R)__builtin_inff();
    return lp;
}

// The hit record of shade() (written out again rather than shared: the trace kernels' code stays as it is) and the albedo
// shade's attenuation would take, stored to the requested outputs.
template <class R>
__device__ __forceinline__ void query_store(const QueryArgs<R>& A, uint32_t j, V<R> o, V<R> d, R time, R tbest, int ibest) {
    typedef typename VecOf<R>::type r4;
    if (A.hit) A.hit[j] = ibest >= 0 ? 1u : 0u;
    if (A.kind == kQueryAny) return;
    V<R> pt{0, 0, 0}, nrm{0, 0, 0}, alb{0, 0, 0};
    bool front = false;
    int mat_out = -1;
    if (ibest >= 0) {
        uint32_t mat_idx;
        if ((uint32_t)ibest < A.sc.n_spheres) {
            const r4 q = A.sc.sph_pool[2 * ibest], w4 = A.sc.sph_pool[2 * ibest + 1];
            sphere_hit_record<R>(q, w4, o, d, time, tbest, pt, nrm);
            mat_idx = bits(w4.w);
        } else {
            const uint32_t ti = (uint32_t)ibest - A.sc.n_spheres;
            const r4 a = A.sc.tri[3 * ti], b = A.sc.tri[3 * ti + 1], c = A.sc.tri[3 * ti + 2];
            pt = {fm(d.x, tbest, o.x), fm(d.y, tbest, o.y), fm(d.z, tbest, o.z)};
            nrm = unit(cross3(V<R>{b.x, b.y, b.z}, V<R>{c.x, c.y, c.z}));
            mat_idx = bits(a.w);
        }
        front = face_forward<R>(d, nrm);
        const r4 m = A.sc.mat[mat_idx];
        alb = (bits(m.x) & 0xffu) == 2u ? V<R>{R(1), R(1), R(1)} : texture_value<R>(A.sc.tex, bits(m.y), pt);
        mat_out = (int)mat_idx;
    }
    if (A.index) A.index[j] = ibest;
    if (A.t) A.t[j] = ibest >= 0 ? tbest : (R)__builtin_inff();
    if (A.point) A.point[3ull * j] = pt.x, A.point[3ull * j + 1] = pt.y, A.point[3ull * j + 2] = pt.z;
    if (A.normal) A.normal[3ull * j] = nrm.x, A.normal[3ull * j + 1] = nrm.y, A.normal[3ull * j + 2] = nrm.z;
    if (A.front) A.front[j] = front ? 1u : 0u;
    if (A.material) A.material[j] = mat_out;
    if (A.albedo) A.albedo[3ull * j] = alb.x, A.albedo[3ull * j + 1] = alb.y, A.albedo[3ull * j + 2] = alb.z;
}

// Flat list: one ray per lane, the wave streams every sphere class and the triangles exactly as trace_kernel does.  The scan is
// wave-uniform over the list, so ANY gains nothing from stopping one lane; the wave skips the triangle stream when all of its
// lanes already have a hit.  Lanes past the batch trace its last ray (full EXEC in the scan) and store nothing.
template <class R> __global__ __launch_bounds__(256, 4) void query_kernel(const QueryArgs<R> A) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool valid = i < A.n;
    V<R> o, d;
    R time, tmax;
    const uint32_t j = query_ray<R>(A, valid ? i : A.n - 1u, o, d, time, tmax);
    ScanRay<R> ray[1];
    const V<R> ud = unit(d);
    scan_begin<R, 1>(ray[0], o, d, ud, time);
    ray[0].tbest = tmax;
    scan_sphere_classes<R, 1>(A.sc, ray, A.tmin);
    narrow_flush<R, 1>(A.sc, ray, A.tmin);
    if (A.kind != kQueryAny || __ballot(ray[0].ibest < 0) != 0ull) scan_triangles<R, 1>(A.sc, ray, A.tmin);
    if (valid) query_store<R>(A, j, o, d, time, ray[0].tbest, ray[0].ibest);
}

// BVH: one ray per lane, the render's walk — box steps from the LDS copy of the tree's top and from global memory, per-lane
// stacks in LDS, the oversized hittables first, then rounds of (N) box steps, (L) leaf reject tests, (C) f64 roots.  Persistent
// workgroups (one per CU, as trace_kernel_bvh: one copy of the top serves the CU) take the batch 64 rays per wave at a time from
// a counter: a wave's 64 consecutive rays are one 8x8 pixel tile in the camera form.  ANY ends a lane's walk at its first
// accepted root.  (No lane refill inside a batch: the lanes of a wave finish together or idle)
template <class R, bool QUANT> __global__ __launch_bounds__(RAYZ_BVH_WG, (bvh_waves<R>() * 256 >= RAYZ_BVH_WG ? bvh_waves<R>() * 256 / RAYZ_BVH_WG : 1))
void query_kernel_bvh(const QueryArgs<R> A) {
    typedef typename VecOf<R>::type r4;
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t n_nodes = A.sc.bvh_n_nodes;
    const float tmin32 = round_down_f32(A.tmin);
    const bool any_kind = A.kind == kQueryAny;
    extern __shared__ uint32_t lds_words[]; // (the set-up and the oversized hittables' pre-walk: trace_kernel_bvh's, restated)
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)lds_words != 0u) {
        if (threadIdx.x == 0) A.counters[31] = 1ull;
        return;
    }
    f4* top = (f4*)lds_words;
    uint32_t* stack = lds_words + A.bvh_top_words + kBvhWg + threadIdx.x;
    for (uint32_t k = threadIdx.x; k < A.sc.bvh_top / 16u; k += kBvhWg) top[k] = A.sc.bvh_nodes[k];
    const f4* nodes_base = scalar_base(A.sc.bvh_nodes);
    stack[0] = kBvhDone;
    unsigned char* big_lds = (unsigned char*)(lds_words + A.bvh_big_words);
    if (threadIdx.x < 2u * A.sc.bvh_n_big_leaves) {
        const uint32_t desc = A.sc.bvh_big[threadIdx.x >> 1], jj = threadIdx.x & 1u;
        if (jj < (desc & 3u)) {
            const uint32_t slot = (desc >> 4) + jj;
            d4* dst64 = (d4*)(big_lds + threadIdx.x * bvh_big_entry_bytes<R>());
            dst64[0] = A.sc.bvh_sph64[2 * slot];
            dst64[1] = A.sc.bvh_sph64[2 * slot + 1];
            r4* dst = (r4*)(dst64 + 2);
            const r4* rec = A.sc.bvh_leaf + (size_t)A.sc.bvh_leaf_stride * slot;
            dst[0] = rec[0];
            dst[1] = rec[1];
            dst[2] = A.sc.bvh_leaf_stride > 2u ? rec[2] : rec[1];
        }
    }
    __syncthreads();
    uint32_t node_tests = 0, sphere_tests = 0;
#ifdef RAYZ_BVH_PROFILE // (the measurement build's box step times its node fetch: counted, not reported, for queries)
    unsigned long long fetch_ticks = 0;
#define RAYZ_QUERY_FETCH , fetch_ticks
#else
#define RAYZ_QUERY_FETCH
#endif
    BvhQuery<R> q;
    for (;;) {
        unsigned long long base = 0;
        if (lane == 0) base = atomicAdd(&A.counters[0], 64ull);
        base = __shfl(base, 0);
        if (base >= (unsigned long long)A.n) break;
        const uint32_t i = (uint32_t)base + lane;
        const bool valid = i < A.n;
        V<R> o, d;
        R time, tmax;
        const uint32_t j = query_ray<R>(A, valid ? i : A.n - 1u, o, d, time, tmax);
        const V<R> ud = unit(d);
        bvh_begin<R, QUANT>(q, A.sc, o, d, ud, valid ? n_nodes : 0u);
        q.tbest = tmax;
        q.tb32 = round_up_f32(tmax);
        if (A.sc.bvh_n_big_leaves != 0u && valid) {
            for (uint32_t k = 0; k < A.sc.bvh_n_big_leaves; ++k) {
                const uint32_t desc = A.sc.bvh_big[k];
                sphere_tests += desc & 3u;
                for (uint32_t jj = 0; jj < (desc & 3u); ++jj) {
                    const d4* rec64 = (const d4*)(big_lds + (2u * k + jj) * bvh_big_entry_bytes<R>());
                    const r4* rec = (const r4*)(rec64 + 2);
                    const r4 c = rec[0], v = rec[1], w = rec[2];
                    if (bvh_leaf_eval<R>(A.sc, q, desc, jj, c, v, o, d, ud, time, A.tmin, &w) != 0u)
                        bvh_candidate_eval<R>(q, rec64[0], rec64[1], (int)bits(v.w), o, d, time, A.tmin);
                }
            }
        }
        if (any_kind && q.ibest >= 0) q.cur = kBvhDone;
        for (;;) {
            if constexpr (sizeof(R) == 8) q.tb32 = round_up_f32(q.tbest);
            bool can_step = q.cur < kBvhDone;
            int n_can = __popcll(__ballot(can_step));
            bool run = n_can != 0 && (n_can >= kBvhKeepStepping || __ballot((int32_t)q.cur < 0) == 0ull);
            while (run) {
                if (can_step) bvh_node_step<R, kBvhWg, QUANT>(A.sc, nodes_base, q, tmin32, stack RAYZ_QUERY_FETCH);
                {
                    const bool again = q.cur < kBvhDone;
                    node_tests += 2u * (uint32_t)__popcll(__ballot(again));
                    if (again) bvh_node_step<R, kBvhWg, QUANT>(A.sc, nodes_base, q, tmin32, stack RAYZ_QUERY_FETCH);
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
                bvh_leaf_pair<R>(A.sc, q, leaf, o, d, ud, time, A.tmin, cand0, cand1, pool0, pool1);
            }
            if (__ballot((cand0 | cand1) != 0u) != 0ull) bvh_candidate_passes<R>(A.sc, q, cand0, cand1, pool0, pool1, o, d, time, A.tmin);
            if (any_kind && q.ibest >= 0) q.cur = kBvhDone; // occlusion: the first accepted root ends the walk
            if (__ballot(q.cur != kBvhDone) == 0ull) break;
        }
        if (valid) query_store<R>(A, j, o, d, time, q.tbest, q.ibest);
    }
    unsigned long long t2 = sphere_tests;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) t2 += __shfl_xor(t2, off);
    if (lane == 0) {
        atomicAdd(&A.counters[2], (unsigned long long)node_tests);
        atomicAdd(&A.counters[3], t2);
    }
}

// The bound check in front of a query (rayz_hip_scene_query): max |origin| (f64), the smallest and largest time, and flags —
// 1: a NaN or infinite origin, direction or time; 2: a zero direction; 4: a NaN tmax; 8: an origin component beyond
// RAYZ_QUERY_MAX_ORIGIN (tested before the norm is formed, so the norm cannot overflow); 16: a non-zero direction whose largest
// |component| lies outside [RAYZ_QUERY_MIN_DIR, RAYZ_QUERY_MAX_DIR] (include/rayz_hip.h: beyond that range the query arithmetic
// loses true hits).  out[0], out[kQueryBoundStride],
// out[2 kQueryBoundStride] hold order-preserving u64 keys (query_key) for atomicMax / atomicMin, out[3 kQueryBoundStride] the
// flags: one 128-byte line each, so that the four words' atomics do not queue behind one another.  A workgroup reduces in LDS first
// and sends ONE atomic per word (same-address atomics serialise: one per wave cost ≈0.2 ms on a 2·10^6-ray batch).  The host
// resets the words and reads them back.
constexpr uint32_t kQueryBoundStride = 16;
__device__ __forceinline__ unsigned long long query_key(double x) {
    const unsigned long long b = __builtin_bit_cast(unsigned long long, x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
template <class R> __global__ __launch_bounds__(256) void query_bounds_kernel(const R* rays, uint32_t n, unsigned long long* out) {
    __shared__ unsigned long long red[4][4]; // [wave][word]
    unsigned long long omax = query_key(0.0), tlo = query_key(__builtin_inf()), thi = query_key(-__builtin_inf()), flags = 0;
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const R* r = rays + 8ull * i;
        const double ox = r[0], oy = r[1], oz = r[2], tm = r[3], dx = r[4], dy = r[5], dz = r[6], tx = r[7];
        const bool finite = __builtin_isfinite(ox) && __builtin_isfinite(oy) && __builtin_isfinite(oz) && __builtin_isfinite(tm) &&
                            __builtin_isfinite(dx) && __builtin_isfinite(dy) && __builtin_isfinite(dz);
        const double lim = RAYZ_QUERY_MAX_ORIGIN;
        const bool near = __builtin_fabs(ox) <= lim && __builtin_fabs(oy) <= lim && __builtin_fabs(oz) <= lim;
        if (!finite) flags |= 1ull;
        if (dx == 0.0 && dy == 0.0 && dz == 0.0) flags |= 2ull;
        if (tx != tx) flags |= 4ull;
        if (finite && !near) flags |= 8ull;
        const double dm = __builtin_fmax(__builtin_fabs(dx), __builtin_fmax(__builtin_fabs(dy), __builtin_fabs(dz)));
        if (finite && dm != 0.0 && (dm < RAYZ_QUERY_MIN_DIR || dm > RAYZ_QUERY_MAX_DIR)) flags |= 16ull;
        if (finite && near) {
            const unsigned long long k = query_key(__builtin_sqrt(ox * ox + oy * oy + oz * oz));
            omax = k > omax ? k : omax;
            const unsigned long long kt = query_key(tm);
            tlo = kt < tlo ? kt : tlo;
            thi = kt > thi ? kt : thi;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long a = __shfl_xor(omax, off), b = __shfl_xor(tlo, off), c = __shfl_xor(thi, off);
        omax = a > omax ? a : omax;
        tlo = b < tlo ? b : tlo;
        thi = c > thi ? c : thi;
        flags |= __shfl_xor(flags, off);
    }
    const uint32_t wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) {
        red[wave][0] = omax;
        red[wave][1] = tlo;
        red[wave][2] = thi;
        red[wave][3] = flags;
    }
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (int w = 1; w < 4; ++w) {
            omax = red[w][0] > omax ? red[w][0] : omax;
            tlo = red[w][1] < tlo ? red[w][1] : tlo;
            thi = red[w][2] > thi ? red[w][2] : thi;
            flags |= red[w][3];
        }
        atomicMax(&out[0], omax);
        atomicMin(&out[kQueryBoundStride], tlo);
        atomicMax(&out[2 * kQueryBoundStride], thi);
        atomicOr(&out[3 * kQueryBoundStride], flags);
    }
}

} // namespace rayz_dev
