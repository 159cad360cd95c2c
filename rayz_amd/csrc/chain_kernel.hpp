// chain_kernel.hpp — specular-chain G-buffers (rayz_hip_scene_query_camera_chain): the device code.
//
// Per pixel: the camera query's ray (camera_ray_no_rng), then `findHit` again from every hit on a mirror-like metal or a
// dielectric along the deterministic direction scatter_dir gives with the metal's fuzz taken as 0 and every uniform 1.0 —
// unit(reflect) off a metal, the refraction through glass unless it is totally reflected, never the Fresnel reflection —
// until the ray misses, lands on something that is not followed, or has been followed max_depth times.  The record stored is
// the LAST segment's, as a NEAREST query of that segment writes it, with the albedo multiplied by the tint of the surfaces
// the chain went through; beside it the chain key (which surfaces, in which order), the depth and the first hit's index.
//
// Every segment is the query kernels' own scan (flat list) or walk (BVH): the same device functions in the same order
// (flat_scan.hpp: scan_sphere_classes / narrow_flush / scan_triangles; bvh_walk.hpp: bvh_begin / bvh_node_step / bvh_leaf_pair /
// bvh_candidate_passes), so a chain of depth 0 IS the camera query.  The depth loop is per wave: a lane whose chain has ended
// idles in the walk (its cursor is kBvhDone) or traces its last ray again in the scan (full EXEC) and stores nothing; the wave
// leaves when no lane is active.  Included by rayz_hip.hip; the host side is chain.hpp.
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

namespace rayz_dev {

constexpr uint32_t kChainKeyMul = 0x9E3779B1u;

// Where a chain call's results go, each optional: RayzQueryOutputs' fields, then RayzChainOutputs'.  The kernels read it from DEVICE
// memory where a chain ends or moves on (ChainArgs::out), not from their arguments: eleven pointers among the arguments are 22
// scalar registers the BVH walk would have to carry, or spill, through every segment.
template <class R> struct ChainStores {
    int32_t* index;
    R *t, *point, *normal;
    uint8_t* front;
    int32_t* material;
    R* albedo;
    uint8_t* hit;
    uint32_t* key;
    uint8_t* depth;
    int32_t* first_index;
};
constexpr size_t kChainStoreWords = 11; // pointers of a ChainStores
// Puts a call's ChainStores (as words: one kernel for both precisions) where its kernel reads them — a launch in front of the chain
// kernel's on the same stream, so the call stays asynchronous and needs no host buffer that outlives it.
struct ChainStoreWords {
    unsigned long long w[kChainStoreWords];
};
__global__ __launch_bounds__(64) void chain_outputs_kernel(const ChainStoreWords s, unsigned long long* dst) {
    if (threadIdx.x < kChainStoreWords) dst[threadIdx.x] = s.w[threadIdx.x];
}
template <class R> struct ChainArgs {
    QueryArgs<R> q;       // the camera form (q.rays == NULL, q.kind = nearest): scene, camera, deal, tmin, counters; its output
                          // pointers stay NULL.  counters[1] receives Σ (depth + 1) over the pixels
    const ChainStores<R>* out; // DEVICE memory
    double max_fuzz;      // a metal whose fuzz (as the device holds it, R) exceeds this is not followed
    uint32_t max_depth;   // hits followed at most
};

// The generator of a chain step: every uniform is 1.0, so `reflectance > uniform` never holds.
struct OnesRng {};
template <class R> __device__ __forceinline__ R uniform(OnesRng&) { return R(1); }

// What an ACTIVE lane does with the nearest hit (tbest, ibest) of segment `seg` on ray (o, d, time 0): the hit record as
// query_store forms it, then either the chain ends here — the record is stored to entry j and false returned — or the hit is
// followed: key and tint move on and (o, d) become the next segment's ray.
// A lane carries NO chain state through a segment (the BVH walk sits at its register limit, as query_kernel_bvh's does): an active
// lane has followed exactly `seg` hits, so that is its depth; the first index is stored at segment 0; and the running key and tint
// live in the pixel's own `key` and `albedo` entries, which the lane alone writes and reads back — where the caller asked for
// neither output, neither is computed.
template <class R>
__device__ __forceinline__ bool chain_step(const ChainArgs<R>& A, uint32_t j, uint32_t seg, V<R>& o, V<R>& d, V<R> ud, R time, R tbest,
                                           int ibest) {
    typedef typename VecOf<R>::type r4;
    const QueryArgs<R>& Q = A.q;
    // (the entry's addresses are formed HERE: left to itself the compiler forms all of them in front of the depth loop and keeps
    //  them in vector registers through every walk)
    asm volatile("" : "+v"(j));
    const RAYZ_GLOBAL ChainStores<R>* P = (const RAYZ_GLOBAL ChainStores<R>*)A.out; // (.. and the pointers fetched here, likewise)
    asm volatile("" : "+s"(P));
    V<R> pt{0, 0, 0}, nrm{0, 0, 0}, alb{0, 0, 0}, nd{0, 0, 0};
    bool front = false, follow = false;
    int mat_out = -1;
    if (seg == 0u && P->first_index) P->first_index[j] = ibest;
    if (ibest >= 0) {
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
        front = face_forward<R>(d, nrm);
        const r4 m = Q.sc.mat[mat_idx];
        const uint32_t kind = bits(m.x) & 0xffu, method = (bits(m.x) >> 8) & 0xffu;
        alb = kind == 2u ? V<R>{R(1), R(1), R(1)} : texture_value<R>(Q.sc.tex, bits(m.y), pt);
        mat_out = (int)mat_idx;
        const bool specular = kind == 2u || (kind == 1u && !((double)m.z > A.max_fuzz));
        if (specular && seg < A.max_depth) {
            OnesRng g;
            follow = scatter_dir<R>(kind, method, kind == 1u ? R(0) : m.z, m.w, g, d, ud, pt, nrm, front, nd); // false: absorbed
        }
    }
    if (P->albedo) { // tint ⊙ albedo: the next tint of a followed hit, the albedo output of the last one (the tint starts at 1: 1·x = x)
        if (seg != 0u) {
            const V<R> tint{P->albedo[3ull * j], P->albedo[3ull * j + 1], P->albedo[3ull * j + 2]};
            alb = {tint.x * alb.x, tint.y * alb.y, tint.z * alb.z};
        }
        P->albedo[3ull * j] = alb.x, P->albedo[3ull * j + 1] = alb.y, P->albedo[3ull * j + 2] = alb.z;
    }
    if (P->key && (follow || seg == 0u)) P->key[j] = follow ? (seg != 0u ? P->key[j] : 0u) * kChainKeyMul + (uint32_t)(ibest + 1) : 0u;
    if (follow) {
        o = pt;
        d = nd;
        return true;
    }
    if (P->hit) P->hit[j] = ibest >= 0 ? 1u : 0u;
    if (P->index) P->index[j] = ibest;
    if (P->t) P->t[j] = ibest >= 0 ? tbest : (R)__builtin_inff();
    if (P->point) P->point[3ull * j] = pt.x, P->point[3ull * j + 1] = pt.y, P->point[3ull * j + 2] = pt.z;
    if (P->normal) P->normal[3ull * j] = nrm.x, P->normal[3ull * j + 1] = nrm.y, P->normal[3ull * j + 2] = nrm.z;
    if (P->front) P->front[j] = front ? 1u : 0u;
    if (P->material) P->material[j] = mat_out;
    if (P->depth) P->depth[j] = (uint8_t)seg;
    return false;
}

// Σ over the wave of a per-lane count.
__device__ __forceinline__ unsigned long long chain_wave_sum(uint32_t v) {
    unsigned long long s = v;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    return s;
}

// Flat list: one pixel per lane, every segment the scan of query_kernel (XZ form).  Lanes past the frame trace its last pixel's
// camera ray and store nothing.
template <class R> __global__ __launch_bounds__(256, 4) void chain_kernel(const ChainArgs<R> A) {
    __shared__ unsigned int block_segments;
    if (threadIdx.x == 0) block_segments = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const bool valid = i < A.q.n;
    V<R> o, d;
    R time, tmax;
    const uint32_t j = query_ray<R>(A.q, valid ? i : A.q.n - 1u, o, d, time, tmax);
    bool active = valid;
    uint32_t segments = 0;
    for (uint32_t seg = 0;; ++seg) {
        ScanRay<R> ray[1];
        const V<R> ud = unit(d);
        scan_begin<R, 1>(ray[0], o, d, ud, time);
        ray[0].tbest = tmax;
        scan_sphere_classes<R, 1>(A.q.sc, ray, A.q.tmin);
        narrow_flush<R, 1>(A.q.sc, ray, A.q.tmin);
        scan_triangles<R, 1>(A.q.sc, ray, A.q.tmin);
        segments += (uint32_t)__popcll(__ballot(active)); // (wave-uniform)
        if (active) active = chain_step<R>(A, j, seg, o, d, ud, time, ray[0].tbest, ray[0].ibest);
        if (__ballot(active) == 0ull) break;
    }
    if ((threadIdx.x & 63u) == 0u) atomicAdd(&block_segments, segments);
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(&A.q.counters[1], (unsigned long long)block_segments);
}

// BVH: persistent workgroups, 64 pixels (one 8x8 tile) per wave at a time, every segment the walk of query_kernel_bvh — the LDS
// copy of the tree's top, per-lane stacks in LDS, the oversized hittables first, then rounds of box steps, leaf reject tests and
// f64 roots.  A lane whose chain has ended starts no walk (bvh_begin with no node: its cursor is kBvhDone).  ONE loop over the
// segments of all the wave's tiles: a wave with no active lane takes its next 64 pixels (a depth loop inside the tile loop
// compiles to a kernel with a scratch frame).
template <class R, bool QUANT> __global__ __launch_bounds__(RAYZ_BVH_WG, (bvh_waves<R>() * 256 >= RAYZ_BVH_WG ? bvh_waves<R>() * 256 / RAYZ_BVH_WG : 1))
void chain_kernel_bvh(const ChainArgs<R> A) {
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
    uint32_t node_tests = 0, sphere_tests = 0, segments = 0;
#ifdef RAYZ_BVH_PROFILE // (the measurement build's box step times its node fetch: counted, not reported, as for queries)
    unsigned long long fetch_ticks = 0;
#define RAYZ_CHAIN_FETCH , fetch_ticks
#else
#define RAYZ_CHAIN_FETCH
#endif
    BvhQuery<R> q;
    V<R> o{R(0), R(0), R(0)}, d{R(0), R(0), R(1)};
    R time = R(0), tmax = (R)__builtin_inff();
    uint32_t j = 0, seg = 0;
    bool active = false;
    for (;;) {
        if (__ballot(active) == 0ull) { // the wave's pixels are done (or it has none yet): the next 64
            unsigned long long base = 0;
            if (lane == 0) base = atomicAdd(&Q.counters[0], 64ull);
            base = __shfl(base, 0);
            if (base >= (unsigned long long)Q.n) break;
            const uint32_t i = (uint32_t)base + lane;
            active = i < Q.n;
            j = query_ray<R>(Q, active ? i : Q.n - 1u, o, d, time, tmax);
            seg = 0;
        }
        {
            const V<R> ud = unit(d);
            bvh_begin<R, QUANT>(q, Q.sc, o, d, ud, active ? n_nodes : 0u);
            q.tbest = tmax;
            q.tb32 = round_up_f32(tmax);
            if (Q.sc.bvh_n_big_leaves != 0u && active) {
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
                    if (can_step) bvh_node_step<R, kBvhWg, QUANT>(Q.sc, nodes_base, q, tmin32, stack RAYZ_CHAIN_FETCH);
                    {
                        const bool again = q.cur < kBvhDone;
                        node_tests += 2u * (uint32_t)__popcll(__ballot(again));
                        if (again) bvh_node_step<R, kBvhWg, QUANT>(Q.sc, nodes_base, q, tmin32, stack RAYZ_CHAIN_FETCH);
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
            segments += (uint32_t)__popcll(__ballot(active)); // (wave-uniform, as node_tests)
            if (active) active = chain_step<R>(A, j, seg, o, d, ud, time, q.tbest, q.ibest);
            ++seg;
        }
    }
    const unsigned long long t2 = chain_wave_sum(sphere_tests);
    if (lane == 0) {
        atomicAdd(&Q.counters[1], (unsigned long long)segments);
        atomicAdd(&Q.counters[2], (unsigned long long)node_tests);
        atomicAdd(&Q.counters[3], t2);
    }
}
#undef RAYZ_CHAIN_FETCH

} // namespace rayz_dev
