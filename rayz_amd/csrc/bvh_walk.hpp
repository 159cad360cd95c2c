// bvh_walk.hpp — the BVH walk of one lane: the workgroup and LDS constants, the per-lane query (BvhQuery, bvh_begin), the
// conservative f32 slab test (bvh_box_hit), the branch-free box step (bvh_node_step), the parked leaves' reject
// tests (bvh_leaf_eval, bvh_leaf_pair) and the candidates' f64 roots (bvh_candidate, bvh_candidate_passes).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.hpp"
#include "device_types.hpp"
#include "flat_scan.hpp"

namespace rayz_dev {

// ---- BVH traversal (src/hit.zig:181-216) ---------------------------------------------------------------
// The reference recurses left-then-right with a shrinking tmax.  Here each lane walks the same tree with a small
// stack (LDS) and visits the NEARER child first; the nearest hit and its tie rule do not depend on visiting
// order, so the result is the reference's.  Per-lane state of one query:
// Threads per workgroup of the one-path BVH kernel = stride of its LDS stacks.  1,024 = ONE workgroup per CU (16 waves, 4
// per SIMD as before), so that ONE copy of the tree's top serves the whole CU and can take all the LDS the stacks leave:
// ≈1,300 inner-node records for config 3 instead of 256 per 256-thread workgroup.  The walk's shared bottleneck is the
// vector-memory address pipe (TA_TA_BUSY 84 %: every step gathers 64 B per lane, 4 divergent dwordx4 loads); a node read
// from LDS does not go through it.  config 3: 42 % of the lane-steps are served by a 256-record top, 55 % by 1,280
// (profiles/r03/lds_top/): 3,554 instead of 3,366 Msamples/s; same speed as 256-thread workgroups at equal top size.
#ifndef RAYZ_BVH_WG
#define RAYZ_BVH_WG 1024
#endif
constexpr uint32_t kBvhWg = RAYZ_BVH_WG;
// LDS a BVH workgroup may ask for: hipFuncSetAttribute(MaxDynamicSharedMemorySize) refuses requests near the CU's 160 KB
// (151,552 B accepted, 155,648 B refused when probed in round 2; rounds 3-4 ran every BVH render with 153,600 B), so the top of
// the tree is sized for 150 KB in all.  A stack that refuses that is not fatal: render_impl retries with a shorter prefix
// of the top, 8 KB at a time (tests/test_bvh.py exercises the retry through RAYZ_DEBUG_LDS_PAD).
constexpr size_t kBvhLdsBudget = 150 * 1024;
// .. of which this much, after the stacks, holds the oversized hittables' records (the filter record's three words in R and
// the f64 sphere record, per entry; at most 4 descriptors of 2): the per-segment set-up reads them from LDS, not through
// two dependent trips to the L2
constexpr uint32_t kBvhBigEntries = 8;
template <class R> constexpr uint32_t bvh_big_entry_bytes() { return 2u * (uint32_t)sizeof(d4) + 4u * (uint32_t)sizeof(typename VecOf<R>::type); } // (f64 record first: 32-byte aligned)
constexpr size_t kBvhBigLdsBytes = kBvhBigEntries * (2 * 32 + 4 * 32);
constexpr int kBvhStackDepth = 32;            // ≥ tree depth: the halving tree's ceil(log2(n / 2)) + 1 (n ≤ 2^27) + the SAH build's
                                              // 4 extra levels (bvh_build.hpp); (32 + 3) rows of 4 KB still fit kBvhLdsBudget
constexpr uint32_t kBvhDone = 0x7fffffffu;     // cursor: nothing left to visit (positive: not a leaf reference)
constexpr uint32_t kBvhLeafFlag = 0x80000000u; // child reference / stack entry is a leaf descriptor, not an inner index

// Per-lane choices under a wave mask held in scalar registers (bit i = lane i): one vector instruction each.
__device__ __forceinline__ uint32_t mask_select(unsigned long long m, uint32_t if_set, uint32_t if_clear) {
    uint32_t r;
    asm volatile("v_cndmask_b32_e64 %0, %1, %2, %3" : "=v"(r) : "v"(if_clear), "v"(if_set), "s"(m));
    return r;
}
__device__ __forceinline__ uint32_t mask_add(uint32_t x, unsigned long long m) { // x + (the lane's bit of m)
    uint32_t r;
    unsigned long long carry;
    asm volatile("v_addc_co_u32_e64 %0, %1, 0, %2, %3" : "=v"(r), "=s"(carry) : "v"(x), "s"(m));
    return r;
}
__device__ __forceinline__ uint32_t mask_sub(uint32_t x, unsigned long long m) { // x − (the lane's bit of m)
    uint32_t r;
    unsigned long long borrow;
    asm volatile("v_subb_co_u32_e64 %0, %1, %2, 0, %3" : "=v"(r), "=s"(borrow) : "v"(x), "s"(m));
    return r;
}

// max / min of a computed value x and a bound the caller knows is not NaN: the bare instruction.
__device__ __forceinline__ float max_bound(float x, float bound) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(bound));
    return r;
}
// .. the same with a WAVE-UNIFORM bound read straight from a scalar register (as a "v" operand the loop pays a v_mov per step)
__device__ __forceinline__ float max_bound_uniform(float x, float bound) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "s"(bound), "v"(x));
    return r;
}
__device__ __forceinline__ float min_bound(float x, float bound) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(x), "v"(bound));
    return r;
}

template <class R> struct LeafBasis;
template <> struct LeafBasis<float> {
    RayBasis<float> b;
    __device__ __forceinline__ void make(V<float> ud, V<float> o) { b = make_basis<float>(ud, o); }
    __device__ __forceinline__ RayBasis<float> get(V<float>, V<float>) const { return b; }
};
template <> struct LeafBasis<double> {
    __device__ __forceinline__ void make(V<double>, V<double>) {}
    __device__ __forceinline__ RayBasis<float> get(V<double> ud, V<double> o) const {
        return make_basis<float>(V<float>{(float)ud.x, (float)ud.y, (float)ud.z}, V<float>{(float)o.x, (float)o.y, (float)o.z});
    }
};
template <class R> struct BvhQuery {
    // the slab test runs in f32 whatever R is: it only culls, and stays conservative under the conversion (§4.8)
    V<float> qa;    // cell_k / d_k per component (1 / d_k capped, bvh_begin): a slab distance is ONE fma on the plane's
    V<float> qb;    // 16-bit grid index i, t = fm(float(i), qa, qb), with qb = (glo_k − o_k) / d_k
    float tb32;     // tbest as the box steps see it: rounded UP to f32 (refreshed before every run of box steps)
    double inv_a2;  // 1 / (d·d) in f64 for the narrow phase
    R tbest;
    int ibest;      // hittable index
    uint32_t cur;   // what the lane holds: an inner node to visit (< kBvhDone), a parked leaf (kBvhLeafFlag | descriptor),
                    // or kBvhDone — then the stack is empty as well and the walk is complete
    uint32_t sp;    // index of the stack's top entry; entry 0 is a kBvhDone sentinel, so popping an empty stack ends the walk
    uint32_t top;   // the stack's top entry, stack[sp], read AHEAD: every step (and bvh_pop) ends by loading the entry that
                    // will be the top at the next pop, so that a pop takes a register instead of waiting for an LDS round
                    // trip between the box tests and the next node fetch (the walk is latency-bound per wave: 49 % of a
                    // wave's cycles are waits, profiles/r02)
    // the reject test's orthonormal pair, made once per segment by the set-up instead of once per leaf
    // phase (a square root and a division, ≈35 vector instructions, ≈3 times per segment at ≈26 lanes).  R = float only: the
    // f64 kernel sits at 128 VGPRs and keeps making it at the leaves (LeafBasis<double> is empty).
    LeafBasis<R> lb;
};

// The f32 slab test carries NO slack of its own (round 3): the boxes the device holds are padded on the host by
// E = kBoxPadUlps·u·max(S, B) per side (u = 2^-24; S = bound on every ray origin, B = largest box coordinate) before
// they are rounded outward to f32 — see bvh_box_hit for why that makes the test conservative.
constexpr double kBoxPadUlps = 16.0;
// a tree gets 32-byte records of 16-bit plane indices instead of 64-byte records of f32 planes when it has more than this
// many times the inner nodes the LDS top would hold as f32 planes (DevScene::bvh_nodes; measured in profiles/r03/lds_top)
constexpr size_t kQuantizeAboveTops = 12;
__device__ __forceinline__ float round_up_f32(float v) { return v; }
__device__ __forceinline__ float round_up_f32(double v) { return __double2float_ru(v); }
__device__ __forceinline__ float round_down_f32(float v) { return v; }
__device__ __forceinline__ float round_down_f32(double v) { return __double2float_rd(v); }
// 1 / d_k, held to ±K = ±2^64.  A direction component of 0 (or so small that its reciprocal overflows) must not reach
// the slab test as ±inf: fm(plane, ±inf, −o·(±inf)) is −inf for one plane of a box that straddles 0 and NaN for the
// other, and max(−inf, NaN) = −inf then culls a box the ray lies inside.  (Such directions are not exotic: a diffuse
// scatter at |p_k| = 50 returns exactly 0 in one component about once in 10^5 bounces, when the offset is absorbed by the
// rounding of p_k + r_k.)  With the clamp the ray is treated as one whose component is 1 / K: finite distances of the
// right sign (the host's padding of the boxes covers their rounding: bvh_box_hit).
constexpr float kInvCap = 0x1p64f;
__device__ __forceinline__ float capped_inverse(float dk) { // (one v_med3_f32 behind the division)
    return __builtin_amdgcn_fmed3f(1.0f / dk, -kInvCap, kInvCap);
}
// (kGrid = false — a kernel whose records hold f32 planes: the grid is origin 0, cell 1, so qa = inv and qb = noi exactly;
//  the six operations and the grid's kernel arguments are skipped)
template <class R, bool kGrid = true, class SC>
__device__ __forceinline__ void bvh_begin(BvhQuery<R>& q, const SC& sc, V<R> o, V<R> d, V<R> ud, uint32_t n_inner) {
    q.lb.make(ud, o);
    V<float> inv;
    if constexpr (sizeof(R) == 8) { // d_k narrowed to f32 first; a component beyond f32's range would make inv 0: held to ±2^100
        inv = {capped_inverse(__builtin_amdgcn_fmed3f((float)d.x, -0x1p100f, 0x1p100f)),
               capped_inverse(__builtin_amdgcn_fmed3f((float)d.y, -0x1p100f, 0x1p100f)),
               capped_inverse(__builtin_amdgcn_fmed3f((float)d.z, -0x1p100f, 0x1p100f))};
    } else {
        inv = {capped_inverse(d.x), capped_inverse(d.y), capped_inverse(d.z)};
    }
    // −o·inv with the origin at full precision, rounded once; then the grid folded in: a plane with index i lies at
    // glo + i·cell, so its distance (glo + i·cell − o)·inv is fm(i, cell·inv, fm(glo, inv, −o·inv))
    const V<float> noi{(float)(-(o.x * (R)inv.x)), (float)(-(o.y * (R)inv.y)), (float)(-(o.z * (R)inv.z))};
    if constexpr (kGrid) {
        q.qa = {sc.bvh_cell[0] * inv.x, sc.bvh_cell[1] * inv.y, sc.bvh_cell[2] * inv.z};
        q.qb = {fm(sc.bvh_glo[0], inv.x, noi.x), fm(sc.bvh_glo[1], inv.y, noi.y), fm(sc.bvh_glo[2], inv.z, noi.z)};
    } else {
        q.qa = inv;
        q.qb = noi;
    }
    const double ddx = d.x, ddy = d.y, ddz = d.z;
    q.inv_a2 = 1.0 / fm(ddz, ddz, fm(ddy, ddy, ddx * ddx));
    q.tbest = (R)__builtin_inff();
    q.tb32 = __builtin_inff();
    q.ibest = -1;
    q.cur = n_inner ? 0u : kBvhDone;
    q.sp = 0;
    q.top = kBvhDone; // = stack[0], the sentinel
}

// Slab test (AABB.hit, src/hit.zig:70-98) of one child box held as three words of 16-bit grid indices (lower | upper << 16
// per axis): each plane distance is one conversion + one fma, t = fm(float(index), qa_k, qb_k), and the test is bare:
// t1 ≥ t0.  It is CONSERVATIVE — rounding never culls a box the f64 narrow phase would hit — because the BOX carries the
// slack, not the comparison.  With inv = (1/d)(1+e1), noi = −o·inv(1+e2), qa = cell·inv(1+e4), qb = (glo·inv + noi)(1+e5)
// and the fma's own rounding e3, the distance computed for index i is the EXACT distance of the true ray to a plane p' with
//     p' − o = (1+e1)(1+e3)·[i·cell(1+e4) + (glo − o − o·e2)(1+e5)]
//     |p' − p| ≤ (|e1|+|e3|)|p − o| + |e4|·i·cell + |e5||glo − o| + |e2||o|   (+ second order),   p = glo + i·cell
// every |e| ≤ u = 2^-24 except |e1| ≤ 2u for R = double (d_k narrowed to f32, then divided): |p' − p| ≤ 4u(B + S) + u·X + u(B + S)
// + u·S < 7u·(max(S, B) + X) for box coordinates |p|, |glo| ≤ B, origins |o| ≤ S and a grid of extent X.  The host picks
// each lower index as the LARGEST whose plane lies at or below the true plane − E, each upper one as the SMALLEST at or above
// the true plane + E, E = 16u·(max(S, B) + X) (rayz_hip.hip: quantize_box), so each computed slab interval contains the true
// box's exact one, for either sign of d_k.  A direction component of 0 reaches here as ±1/K (bvh_begin): huge finite
// distances whose SIGN is right as long as the origin is not within rounding (< E) of the plane — and a true ray that
// runs parallel to a slab is inside it only if it is strictly between the TRUE planes, i.e. at least E inside the held ones.
// `tmin` is the caller's tmin rounded DOWN to f32, q.tb32 tbest rounded UP.  Returns the entry distance through `t0`.
template <class R, bool kUniformTmin>
__device__ __forceinline__ bool bvh_box_hit_planes(V<float> lo, V<float> hi, const BvhQuery<R>& q, float tmin, float& t0);
__device__ __forceinline__ float plane_lo(uint32_t w) { // float(w & 0xffff): one v_cvt_f32_u32 with a 16-bit source select
    float r;
    asm("v_cvt_f32_u32_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0" : "=v"(r) : "v"(w));
    return r;
}
__device__ __forceinline__ float plane_hi(uint32_t w) { // float(w >> 16)
    float r;
    asm("v_cvt_f32_u32_sdwa %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_1" : "=v"(r) : "v"(w));
    return r;
}
template <class R, bool kUniformTmin = false>
__device__ __forceinline__ bool bvh_box_hit(uint32_t wx, uint32_t wy, uint32_t wz, const BvhQuery<R>& q, float tmin, float& t0) {
    return bvh_box_hit_planes<R, kUniformTmin>(V<float>{plane_lo(wx), plane_lo(wy), plane_lo(wz)},
                                               V<float>{plane_hi(wx), plane_hi(wy), plane_hi(wz)}, q, tmin, t0);
}
// .. of a box held as f32 planes (glo = 0, cell = 1: qa = 1/d, qb = −o/d, and a plane is its own "index")
template <class R, bool kUniformTmin>
__device__ __forceinline__ bool bvh_box_hit_planes(V<float> lo, V<float> hi, const BvhQuery<R>& q, float tmin, float& t0) {
    const float ax = fm(lo.x, q.qa.x, q.qb.x), bx = fm(hi.x, q.qa.x, q.qb.x);
    const float ay = fm(lo.y, q.qa.y, q.qb.y), by = fm(hi.y, q.qa.y, q.qb.y);
    const float az = fm(lo.z, q.qa.z, q.qb.z), bz = fm(hi.z, q.qa.z, q.qb.z);
    // (tmin and tbest are never NaN: max_bound / min_bound spare the canonicalising copy fmax / fmin would put in front of
    // every use — two vector instructions per step)
    // (kUniformTmin: the trace kernels' tmin is the launch's, the same for every lane; the known-answer kernel's is per record)
    t0 = mx(mx(mn(ax, bx), mn(ay, by)), kUniformTmin ? max_bound_uniform(mn(az, bz), tmin) : max_bound(mn(az, bz), tmin));
    float tb;
    if constexpr (sizeof(R) == 4) tb = q.tbest; else tb = q.tb32; // (f32: tbest itself — no second register)
    const float t1 = mn(mn(mx(ax, bx), mx(ay, by)), min_bound(mx(az, bz), tb));
    return t1 >= t0;
}

// The node array's base as scalar registers of its own (the step's global loads take it as their SGPR base: read straight
// out of the kernel-argument block under scalar-register pressure, hipcc hands the inline assembly a VGPR pair).
__device__ __forceinline__ const f4* scalar_base(const f4* p) {
    const unsigned long long nb = (unsigned long long)(uintptr_t)p;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)nb), hi = __builtin_amdgcn_readfirstlane((uint32_t)(nb >> 32));
    return (const f4*)(uintptr_t)((unsigned long long)lo | ((unsigned long long)hi << 32));
}
// Phase N — one step of a lane that holds an inner node: fetch the node's record, slab-test both children, push the
// farther hit child (inner index or flagged leaf descriptor alike) and take the nearer one; with nothing hit, take the
// top of the stack instead.  Whatever the lane then holds says what it does next: an inner node → another step, a leaf →
// parked for phase L, kBvhDone (the sentinel under the stack) → walk complete.  Branch-free: the push lands above the
// top when there is nothing to push, the pop is a read every stepping lane makes.  `stack` is this lane's column of
// the workgroup's LDS stack (entry s at stack[s * 256]).
template <class R, uint32_t WG, bool QUANT>
__device__ __forceinline__ void bvh_node_step(const DevScene<R>& sc, const f4* nodes_base, BvhQuery<R>& q, float tmin, uint32_t* stack
#ifdef RAYZ_BVH_PROFILE
                                              , unsigned long long& g_fetch_ticks
#endif
) {
#ifdef RAYZ_BVH_PROFILE
    const unsigned long long tl0 = __builtin_amdgcn_s_memtime();
#endif
    // Both homes of a node — the LDS copy of the tree's top (at LDS address 0), global memory for the rest — are read
    // from the SAME 32-bit offset (the reference itself): the lanes of either kind take turns under exec, into the same
    // registers.  Two vector instructions (a compare, a shift) instead of the nine a flat-address select costs.
    // (an inner reference IS its record's byte offset, index << 6 or << 5: the host keeps the node count below 2^25;
    //  sc.bvh_top is a byte count likewise — no shift, no second register)
    const unsigned long long in_top = __ballot(q.cur < sc.bvh_top);
    const uint32_t off = q.cur;
    unsigned long long saved;
    float tl, tr;
    bool hl, hr;
    uint32_t l, r; // each child's reference: an inner record's offset, or kBvhLeafFlag | leaf descriptor
    if constexpr (QUANT) {
        u4 nl, nr; // the two children: {x, y, z plane words, reference}
        asm volatile("s_mov_b64 %[sv], exec\n\t"
                     "s_and_b64 exec, %[sv], %[mt]\n\t" // (SCC = some lane: an empty turn is skipped — the memory
                     "s_cbranch_scc0 1f\n\t"            //  pipes would still spend their cycles on it)
                     "ds_read_b128 %[n0], %[off]\n\t"
                     "ds_read_b128 %[n1], %[off] offset:16\n"
                     "1:\n\t"
                     "s_andn2_b64 exec, %[sv], %[mt]\n\t"
                     "s_cbranch_scc0 2f\n\t"
                     "global_load_dwordx4 %[n0], %[off], %[base]\n\t"
                     "global_load_dwordx4 %[n1], %[off], %[base] offset:16\n"
                     "2:\n\t"
                     "s_mov_b64 exec, %[sv]\n\t"
                     "s_waitcnt vmcnt(1) lgkmcnt(1)" // the LEFT child's load (and the stack top read ahead before it)
                     : [n0] "=&v"(nl), [n1] "=&v"(nr), [sv] "=&s"(saved)
                     : [off] "v"(off), [mt] "s"(in_top), [base] "s"(nodes_base)
                     : "memory", "scc");
        hl = bvh_box_hit<R, true>(nl.x, nl.y, nl.z, q, tmin, tl);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(nr) : "v"(tl) : "memory"); // (see the f32 form below)
        hr = bvh_box_hit<R, true>(nr.x, nr.y, nr.z, q, tmin, tr);
        l = nl.w, r = nr.w;
    } else {
        f4 llo, lhi, rlo, rhi;
        asm volatile("s_mov_b64 %[sv], exec\n\t"
                     "s_and_b64 exec, %[sv], %[mt]\n\t"
                     "s_cbranch_scc0 1f\n\t"
                     "ds_read_b128 %[n0], %[off]\n\t"
                     "ds_read_b128 %[n1], %[off] offset:16\n\t"
                     "ds_read_b128 %[n2], %[off] offset:32\n\t"
                     "ds_read_b128 %[n3], %[off] offset:48\n"
                     "1:\n\t"
                     "s_andn2_b64 exec, %[sv], %[mt]\n\t"
                     "s_cbranch_scc0 2f\n\t"
                     "global_load_dwordx4 %[n0], %[off], %[base]\n\t"
                     "global_load_dwordx4 %[n1], %[off], %[base] offset:16\n\t"
                     "global_load_dwordx4 %[n2], %[off], %[base] offset:32\n\t"
                     "global_load_dwordx4 %[n3], %[off], %[base] offset:48\n"
                     "2:\n\t"
                     "s_mov_b64 exec, %[sv]\n\t"
                     "s_waitcnt vmcnt(2) lgkmcnt(2)" // the LEFT child's two loads (and the stack top read ahead before them)
                     : [n0] "=&v"(llo), [n1] "=&v"(lhi), [n2] "=&v"(rlo), [n3] "=&v"(rhi), [sv] "=&s"(saved)
                     : [off] "v"(off), [mt] "s"(in_top), [base] "s"(nodes_base)
                     : "memory", "scc");
        hl = bvh_box_hit_planes<R, true>(V<float>{llo.x, llo.y, llo.z}, V<float>{lhi.x, lhi.y, lhi.z}, q, tmin, tl);
        // .. and the left box is tested while the right child's loads are still on their way (they return in order; the
        // empty dependence on tl keeps the left test above this wait, the "+v" keep the compiler's hands off the registers
        // in flight): +1.7 % config 3, profiles/r03/bvh_step/split_wait.log
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" : "+v"(rlo), "+v"(rhi) : "v"(tl) : "memory");
        hr = bvh_box_hit_planes<R, true>(V<float>{rlo.x, rlo.y, rlo.z}, V<float>{rhi.x, rhi.y, rhi.z}, q, tmin, tr);
        l = bits(llo.w), r = bits(rlo.w);
    }
#ifdef RAYZ_BVH_PROFILE // time from issuing the node fetch to having it (the wave's own view), accumulated in g_prof_fetch
    g_fetch_ticks += __builtin_amdgcn_s_memtime() - tl0;
#endif
    // Which child was hit decides everything below, so the decisions live as WAVE MASKS in scalar registers (the boolean
    // algebra runs on the scalar unit, which has slack; the vector unit, which has none, spends one v_cndmask per choice):
    const unsigned long long ml = __ballot(hl), mr = __ballot(hr), mlt = __ballot(tr < tl);
    const unsigned long long swap = mr & (~ml | mlt), both = ml & mr, none = ~(ml | mr);
    // Nearer child first (a child that was not hit may ride along as `near` or `far`: `none` and `both` decide what is used)
    const uint32_t near = mask_select(swap, r, l);
    uint32_t far = mask_select(swap, l, r);
    q.cur = mask_select(none, q.top, near); // nothing hit => nothing pushed: the entry read ahead IS the top
    // The push goes AFTER that select in program order (the empty asm makes `far` look computed from q.cur): the compiler
    // guards the select's read of q.top — the previous step's read-ahead, long since back behind the node fetch — with
    // s_waitcnt lgkmcnt(0), and a store issued before it would put an LDS round trip into every step's dependent chain.
    asm volatile("" : "+v"(far) : "v"(q.cur));
    stack[WG * (q.sp + 1u)] = far; // lands above the top unless both were hit
    const uint32_t sp = mask_add(q.sp, both);
    q.sp = mask_sub(sp, none); // popping the sentinel leaves sp at −1: the lane holds kBvhDone and steps no more until
                               // bvh_begin (its read-ahead below lands in the guard row under the stack)
    q.top = stack[WG * q.sp]; // read ahead for the NEXT pop — after the store above (LDS keeps a wave's order), consumed
                               // one step later, behind that step's node fetch: its latency is off the critical path
}

// The next entry of a lane that is done with its parked leaf.
template <class R, uint32_t WG> __device__ __forceinline__ void bvh_pop(BvhQuery<R>& q, const uint32_t* stack) {
    q.cur = q.top;
    q.sp -= 1u;
    q.top = stack[WG * q.sp];
}

// The reject test of a leaf entry (general velocity form of DESIGN.md §4.3, f32 for both precisions): the ONE place it is
// written — the BVH kernels' leaves, the oversized hittables and the known-answer entry all call it.
__device__ __forceinline__ bool leaf_reject_test(const RayBasis<float>& b, float ft, V<float> c, V<float> v, float r2_padded) {
    const float p1 = fm(v.z, ft * b.e1z, fm(v.x, ft * b.e1x, basis_p1<float>(b, c.x, c.z)));
    const float p2 = fm(v.z, ft * b.e2z, fm(v.y, ft * b.e2y, fm(v.x, ft * b.e2x, basis_p2<float>(b, c.x, c.y, c.z))));
    return sphere_candidate<float>(p1, p2, r2_padded);
}

// Phase L — entry k of a parked leaf: a triangle is decided here (R arithmetic only); a sphere gets the reject
// test in R and, if its line meets the sphere, is parked as a candidate (slot + 1) for phase C.
// (a sphere's pool index rides in its record's last word, v.w: phase C takes it from there — see bvh_leaf_pair)
template <class R>
__device__ __forceinline__ uint32_t bvh_leaf_eval(const DevScene<R>& sc, BvhQuery<R>& q, uint32_t leaf, uint32_t k, typename VecOf<R>::type c,
                                                  typename VecOf<R>::type v, V<R> o, V<R> d, V<R> ud, R time, R tmin,
                                                  const typename VecOf<R>::type* third_word = nullptr) {
    typedef typename VecOf<R>::type r4;
    const uint32_t slot = (leaf >> 4) + k;
    if ((leaf >> (2u + k)) & 1u) { // triangle
        const r4 e2 = third_word ? *third_word : sc.bvh_leaf[(size_t)sc.bvh_leaf_stride * slot + 2];
        const V<R> v0{c.x, c.y, c.z}, e1{v.x, v.y, v.z}, ee2{e2.x, e2.y, e2.z};
        tri_accept<R>(tri_filter<R>(v0, e1, ee2, o, d), v0, e1, ee2, o, d, tmin, (int)bits(c.w), q.tbest, q.ibest);
        return 0u;
    }
    // the flat list's reject test: in f32 for both precisions, on the ray narrowed to f32 (hipcc shares the basis between
    // both entries of a leaf); c.w = the f32 padded square
    const RayBasis<float> b = q.lb.get(ud, o);
    return leaf_reject_test(b, (float)time, V<float>{(float)c.x, (float)c.y, (float)c.z}, V<float>{(float)v.x, (float)v.y, (float)v.z}, (float)c.w)
               ? slot + 1u : 0u;
}
// Both entries of a parked leaf (phase L): their records are FETCHED together — entry 1's loads do not wait for entry 0's
// test (two dependent memory round trips per leaf phase otherwise); a leaf of one repeats entry 0's address, its second
// result is dropped.  R = float only: the f64 kernel has no eight registers to spare and tests one entry after the other.
// The candidates' POOL indices (the tie rule's and the hit record's key) come back too: they ride in the records just
// fetched (v.w), and phase C would otherwise fetch them again — after its roots, when a root is accepted: the compiler
// sinks that load into the branch, a second memory round trip inside the phase.
template <class R>
__device__ __forceinline__ void bvh_leaf_pair(const DevScene<R>& sc, BvhQuery<R>& q, uint32_t leaf, V<R> o, V<R> d, V<R> ud, R time, R tmin,
                                              uint32_t& cand0, uint32_t& cand1, int& pool0, int& pool1) {
    typedef typename VecOf<R>::type r4;
    const bool two = (leaf & 3u) > 1u;
    if constexpr (sizeof(R) == 4) {
        const r4* rec = sc.bvh_leaf + (size_t)sc.bvh_leaf_stride * (leaf >> 4);
        const r4* rec1 = rec + (two ? sc.bvh_leaf_stride : 0u);
        const r4 c0 = rec[0], v0 = rec[1], c1 = rec1[0], v1 = rec1[1];
        cand0 = bvh_leaf_eval<R>(sc, q, leaf, 0u, c0, v0, o, d, ud, time, tmin);
        pool0 = (int)bits(v0.w);
        if (two) cand1 = bvh_leaf_eval<R>(sc, q, leaf, 1u, c1, v1, o, d, ud, time, tmin);
        pool1 = (int)bits(v1.w);
    } else {
        const r4* rec = sc.bvh_leaf + (size_t)sc.bvh_leaf_stride * (leaf >> 4);
        const r4 c0 = rec[0], v0 = rec[1];
        cand0 = bvh_leaf_eval<R>(sc, q, leaf, 0u, c0, v0, o, d, ud, time, tmin);
        pool0 = (int)bits(v0.w);
        if (two) {
            const r4 c1 = rec[sc.bvh_leaf_stride], v1 = rec[sc.bvh_leaf_stride + 1u];
            cand1 = bvh_leaf_eval<R>(sc, q, leaf, 1u, c1, v1, o, d, ud, time, tmin);
            pool1 = (int)bits(v1.w);
        }
    }
}

// Phase C — a parked sphere candidate: the flat list's narrow phase (narrow_eval) on the candidate's f64 record, into the
// query's nearest hit.  bvh_candidate takes the record from the leaf-ordered f64 copy by the candidate's slot.
template <class R>
__device__ __forceinline__ void bvh_candidate_eval(BvhQuery<R>& q, const d4 c2, const d4 v2, int pool, V<R> o, V<R> d, R time, R tmin) {
    narrow_eval<R>(c2, v2, pool, o, d, time, q.inv_a2, tmin, q.tbest, q.ibest);
}
template <class R>
__device__ __forceinline__ void bvh_candidate(const DevScene<R>& sc, BvhQuery<R>& q, uint32_t slot, int pool, V<R> o, V<R> d, R time,
                                              R tmin) {
    bvh_candidate_eval<R>(q, sc.bvh_sph64[2 * slot], sc.bvh_sph64[2 * slot + 1], pool, o, d, time, tmin);
}

// Phase C of a round, as query_kernel_bvh and experiments/ run it (trace_kernel_bvh restates it: calling this there changes the f64
// kernel's schedule and register allocation, and its machine code is pinned): the f64 roots of phase L's candidates (slot + 1, or
// 0).  A lane's only candidate goes into the first pass whichever entry it came from: the second pass runs only when some lane
// has two (the nearest hit does not depend on the order).
template <class R> __device__ __forceinline__ void bvh_candidate_passes(const DevScene<R>& sc, BvhQuery<R>& q, uint32_t cand0, uint32_t cand1, int pool0, int pool1,
                                                                        V<R> o, V<R> d, R time, R tmin) {
    const uint32_t c0 = cand0 != 0u ? cand0 : cand1, c1 = cand0 != 0u ? cand1 : 0u;
    const int p0 = cand0 != 0u ? pool0 : pool1;
    if (c0 != 0u) bvh_candidate<R>(sc, q, c0 - 1u, p0, o, d, time, tmin);
    if (__ballot(c1 != 0u) != 0ull) {
        if (c1 != 0u) bvh_candidate<R>(sc, q, c1 - 1u, pool1, o, d, time, tmin);
    }
}

// How long a round's phases go on (trace_kernels_bvh.hpp describes the round; the query and chain kernels run its phases too):
constexpr int kBvhKeepActive = 20;   // rounds continue while at least this many lanes still walk
constexpr int kBvhKeepStepping = 18; // phase N continues while at least this many lanes can take a box step
                                     // (defaults; TraceArgs::bvh_keep carries the values in use)

// Waves per SIMD the register allocation of every kernel that walks aims at (the launch bounds of the trace, query and chain
// kernels): 4 (128 VGPRs, nothing spilled).  At 5 (96 VGPRs) the trace kernel spills 54 VGPRs into the box-step loop and is 8 %
// slower; the box steps are issue-bound, not latency-bound (profiles/r02), so the fifth wave buys nothing.
#ifndef RAYZ_BVH_WAVES
#define RAYZ_BVH_WAVES 4
#endif
#ifndef RAYZ_BVH_WAVES_F64 // the f64 kernel fits 128 VGPRs too since its box walk and its reject tests run in f32 (it needed
#define RAYZ_BVH_WAVES_F64 4 // 151 and ran 3 waves per SIMD before: +13 % from the fourth)
#endif
template <class R> constexpr int bvh_waves() { return sizeof(R) == 8 ? RAYZ_BVH_WAVES_F64 : RAYZ_BVH_WAVES; }

} // namespace rayz_dev
