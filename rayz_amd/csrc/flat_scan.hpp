// flat_scan.hpp — the flat hit list's scan: the narrow phase (narrow_eval), the conservative reject test with its two bases
// (RayBasis, make_basis), the triangle test (§4.7), the packed block forms (PackedGroup / ScanGroup) and the scan
// loops over the streams (scan_blocks, scan_sets, scan_plane_class, scan_triangles, scan_spheres).  Wave-uniform over the sphere
// index: records come through the scalar path and feed the VALU as SGPR operands (rayz_device.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.hpp"
#include "device_types.hpp"
#include "plane_runs.hpp"

namespace rayz_dev {

// ---- narrow phase: one candidate that passed the reject test, src/geom.zig:40-61 ------------------
// The reference's quadratic in f64 on the pool's f64 sphere, for the ray as the kernel holds it; the
// chosen root is rounded to R.  Ties in t go to the larger pool index (the reference's "t ≤ maxt, later
// wins" over its flat list, src/hit.zig:208-214), which makes the result independent of the order in which
// candidates are examined — so the flat-list scan only PARKS candidate slots (≤ 4 per ray) and evaluates
// them afterwards for all lanes together, instead of interrupting the scan ~30 times per segment for one or two
// lanes each.
template <class R>
__device__ __forceinline__ void narrow_eval(const d4 c, const d4 v, int pool, V<R> o, V<R> d, R time, double inv_a2, R tmin,
                                            R& tbest, int& ibest) {
    const double dx = d.x, dy = d.y, dz = d.z, tm = time;
    const double qx = fm(v.x, tm, c.x - (double)o.x), qy = fm(v.y, tm, c.y - (double)o.y), qz = fm(v.z, tm, c.z - (double)o.z);
    const double a2 = fm(dz, dz, fm(dy, dy, dx * dx));
    const double hb2 = fm(dz, qz, fm(dy, qy, dx * qx));
    const double cc2 = fm(qz, qz, fm(qy, qy, fm(qx, qx, -c.w)));
    const double disc2 = fm(-a2, cc2, hb2 * hb2);
    if (disc2 >= 0.0) {
        const double rt = __builtin_sqrt(disc2);
        const R t1 = (R)((hb2 - rt) * inv_a2), t2 = (R)((hb2 + rt) * inv_a2);
        const R t = t1 >= tmin ? t1 : t2;
        accept_root<R>(t, pool, tmin, tbest, ibest);
    }
}

// ---- reject test -------------------------------------------------------------------------
// Per ray: an orthonormal pair (e1, e2) perpendicular to the unit direction ud, with e1 in the xz-plane
// (e1.y = 0), e2 = ud × e1, and k = −o·e.  The squared distance from the ray's line to a centre c is
// p1² + p2² with p1 = c·e1 + k1 (2 FMAs; a y-velocity never enters it) and p2 = c·e2 + k2 (3 FMAs), so the test
// r² − p1² − p2² ≥ 0 costs 7 VALU per static sphere, 8 with a y-velocity, 12 with a general one — against
// 10 / 11 / 13 for the textbook (ud·oc)² − (|oc|² − r²), and needs no c − o.
// Which axis e1 avoids is a compile-time fact of a basis (and of the kernel that scans with it).  kBasisXZ is the form above.
// kBasisXY keeps e1 in the xy-plane (e1.z = 0): e1 = (ud.y, −ud.x, 0)/√(ud.x² + ud.y²), e2 = ud × e1.  Its p1 = cx·e1x + cy·e1y + k1
// has no cz term, and in a plane run (one cy) cy·e1y folds into a per-run K1 as cy·e2y folds into K2: a plane sphere costs
// p1 = fm(cx, e1x, K1), p2 = fm(cz, e2z, fm(cx, e2x, K2)) and the disc's two: 5 packed FMAs per sphere pair, not 6.  A loose
// sphere stays at 7, a loose y-moving one pays 9 (vy enters p1 too), a general velocity 12.
constexpr int kBasisXZ = 0, kBasisXY = 1;
template <class R, int AX = kBasisXZ> struct RayBasis {
    R e1x, e1z, e2x, e2y, e2z, k1, k2;
};
template <class R> struct RayBasis<R, kBasisXY> {
    R e1x, e1y, e2x, e2y, e2z, k1, k2;
};
// k1 = −o·e1 of the xy basis, as make_basis rounds it (the scan makes it again after a plane run: scan_plane_class).
template <class R> __device__ __forceinline__ R basis_xy_k1(const RayBasis<R, kBasisXY>& b, R ox, R oy) { return -fm(oy, b.e1y, ox * b.e1x); }
template <class R, int AX = kBasisXZ> __device__ __forceinline__ RayBasis<R, AX> make_basis(V<R> ud, V<R> o) {
    RayBasis<R, AX> b;
    if constexpr (AX == kBasisXY) {
        const R h2 = fm(ud.y, ud.y, ud.x * ud.x);
        b.e1x = R(1);
        b.e1y = R(0);
        if (h2 > R(1e-30)) { // below that (|ud.x|, |ud.y| < 1e-15) the x axis is perpendicular to ud far inside the slack
            const R ih = R(1) / sq(h2);
            b.e1x = ud.y * ih;
            b.e1y = -(ud.x * ih);
        }
        b.e2x = -(ud.z * b.e1y);
        b.e2y = ud.z * b.e1x;
        b.e2z = fm(ud.x, b.e1y, -(ud.y * b.e1x));
        b.k1 = basis_xy_k1<R>(b, o.x, o.y);
    } else {
        const R h2 = fm(ud.z, ud.z, ud.x * ud.x);
        b.e1x = R(1);
        b.e1z = R(0);
        if (h2 > R(1e-30)) { // below that (|ud.x|, |ud.z| < 1e-15) the x axis is perpendicular to ud far inside the slack
            const R ih = R(1) / sq(h2);
            b.e1x = ud.z * ih;
            b.e1z = -(ud.x * ih);
        }
        b.e2x = ud.y * b.e1z;
        b.e2y = fm(ud.z, b.e1x, -(ud.x * b.e1z));
        b.e2z = -(ud.y * b.e1x);
        b.k1 = -fm(o.z, b.e1z, o.x * b.e1x);
    }
    b.k2 = -fm(o.z, b.e2z, fm(o.y, b.e2y, o.x * b.e2x));
    return b;
}
template <class R> __device__ __forceinline__ R basis_p1(const RayBasis<R>& b, R cx, R cz) {
    return fm(cz, b.e1z, fm(cx, b.e1x, b.k1));
}
template <class R> __device__ __forceinline__ R basis_p2(const RayBasis<R>& b, R cx, R cy, R cz) {
    return fm(cz, b.e2z, fm(cy, b.e2y, fm(cx, b.e2x, b.k2)));
}
template <class R> __device__ __forceinline__ R basis_disc(R p1, R p2, R r2) { return fm(-p1, p1, fm(-p2, p2, r2)); }
// The filter is CONSERVATIVE: `r2` is not r² but (r + E)², E = 32·u·(|c| + |v| + r + S) added on the host
// (pad_radius2 in rayz_hip.hip; u = unit roundoff of R, S = bound on every ray origin).  E covers the rounding of
// unit(d), of the basis, of k, p1, p2 and of this expression (derivation: DESIGN.md §4.3), so a sphere whose f64
// discriminant is ≥ 0 always reaches the narrow phase; the narrow phase decides.
template <class R> __device__ __forceinline__ bool sphere_candidate(R p1, R p2, R r2_padded) {
    return basis_disc<R>(p1, p2, r2_padded) >= R(0);
}

// ---- build-defined triangle (Möller–Trumbore in R) ----------------------------------
// Filter value: ≥ 0 iff the barycentrics pass, written without a division or a sign branch:
// su = (s·p)·det, sv = (d·q)·det, w = det² − (su + sv); candidate iff min(su, sv, w) ≥ 0.  There is no f64 phase
// behind it: for triangles this value IS the decision (in R, identically in the oracle), not a pre-filter.
template <class R> __device__ __forceinline__ R tri_filter(V<R> v0, V<R> e1, V<R> e2, V<R> o, V<R> d) {
    const V<R> pv = cross3(d, e2);
    const R det = dot3(e1, pv);
    const V<R> sv{o.x - v0.x, o.y - v0.y, o.z - v0.z};
    const R su = dot3(sv, pv) * det;
    const V<R> qv = cross3(sv, e1);
    const R svv = dot3(d, qv) * det;
    const R w = fm(det, det, -(su + svv));
    return mn(mn(su, svv), w);
}
// Candidate: t = (e2·q) / det, then the same acceptance rule as spheres (nearest, ties to the larger index).
template <class R>
__device__ __forceinline__ void tri_accept(R filt, V<R> v0, V<R> e1, V<R> e2, V<R> o, V<R> d, R tmin, int prim, R& tbest,
                                           int& ibest) {
    if (filt >= R(0)) {
        const V<R> pv = cross3(d, e2);
        const R det = dot3(e1, pv);
        if (det != R(0)) {
            const V<R> sv{o.x - v0.x, o.y - v0.y, o.z - v0.z};
            const V<R> qv = cross3(sv, e1);
            const R t = dot3(e2, qv) / det;
            accept_root<R>(t, prim, tmin, tbest, ibest);
        }
    }
}

// Slots the plane runs of a static / mov-Y stream cover (its head: see DevScene).
__device__ __forceinline__ uint32_t plane_slots(const float* stream) { return ((const RAYZ_CONSTANT uint32_t*)stream)[1]; }

// One scan group of a velocity class, held in SGPRs: load() issues the scalar loads, discs() runs the reject test of its
// spheres against 64 rays.  ready(at) waits for the loads; the stream pointer `at` passes through the same empty asm, so the
// load the scan issues next, at an offset from `at`, depends on the wait and cannot be issued in front of it.
template <class R, int CLS> struct ScanGroup;

// One sphere of a packed block as the host hands it over; the default is the pad sphere (r² = -inf: never a candidate).
template <class R> struct BlockSphere { R cx = R(0), cy = R(0), cz = R(0), r2 = -(R)__builtin_inff(), vy = R(0); };

// The packed block: G spheres, SoA, cx[G] (cy[G]) cz[G] r²[G] (vy[G]).  The static and mov-Y classes, loose and in plane runs,
// are ONE form that differs in two facts: whether a block carries cy (kCy: loose spheres; a plane run holds its height once,
// in the stream's head) and whether it carries vy (kVy: the mov-Y class).  A field a form lacks has no place in the stream,
// is never loaded or read, and costs no register.  The offsets below are the layout's one statement: load() reads by them,
// and the host writes the streams through put().
//
// The reject tests of a block run two spheres per instruction: each stage is ONE packed FMA (v_pk_fma_f32 for
// R = float) whose scalar operand is an SGPR PAIR — the same field of two neighbouring spheres.  Measured on
// gfx950 (tools/ubench): a VALU instruction that reads a different SGPR each time issues at ≈2.75 cycles, not 2,
// so the 7 scalar reads of a test bound the scalar-FMA form at ≈21 ticks per wave-test; the packed form needs
// 3.5 pair reads per test and runs at 14.7.  Every half of a packed FMA is an ordinary IEEE FMA: results are
// bit-identical to the scalar form (and to the oracle).  discs() is written stage by stage across the group's pairs, not
// pair by pair: a packed FMA that reads the result of the one just issued costs gfx950 an s_nop, and in this order hipcc
// finds the other pair's FMA to put between them (the same FMAs on the same values either way).
//
// Plane-run blocks (kCy = false): every sphere of the run has the same cy, so cy·e2y + k2 is ONE value per ray and run, K2,
// which the run loop (scan_plane_class) puts in the basis's k2 before the run: discs() finds it in b.k2.
// p2 = fm(cz, e2z, fm(cx, e2x, K2)): 6 packed FMAs per sphere pair instead of 7 (static), 7 instead of 8 (mov-Y).  The same
// three roundings as basis_p2, in another order, with the same bounds on the partial sums: the pad E stays.
//
// One-radius sets (kR2 = false; rayz_plane::plan_sets): the members of a static run or a speed bucket whose radii
// lie close together are tested with ONE padded r², the set's, which discs() takes as an argument: a loop-invariant operand of
// disc = fm(−p2, p2, R2), the one stage that reads no stream field.  Their blocks are cx[GN] cz[GN], GN = 8: one 16-word load.
template <class R, bool kCy, bool kVy, bool kR2 = true, int GN = group_size<R>()> struct PackedGroup {
    typedef typename VecOf<R>::pair pr;
    static constexpr int G = GN, H = G / 2;
    static constexpr int kWords = 2 + kR2 + kCy + kVy; // words of the stream per sphere
    // word offset of each field inside a block (a field the form lacks: -1)
    static constexpr int kOffCx = 0, kOffCy = kCy ? G : -1, kOffCz = (1 + kCy) * G, kOffR2 = kR2 ? (2 + kCy) * G : -1,
                         kOffVy = kVy ? (2 + kR2 + kCy) * G : -1;
    pr cx[H], cy[H], cz[H], r2[H], vy[H];
    // Host: sphere s at slot k of a section of blocks in this form.
    static void put(R* section, size_t k, const BlockSphere<R>& s = BlockSphere<R>()) {
        R* blk = section + k / G * (kWords * G) + k % G;
        blk[kOffCx] = s.cx, blk[kOffCz] = s.cz;
        if constexpr (kR2) blk[kOffR2] = s.r2;
        if constexpr (kCy) blk[kOffCy] = s.cy;
        if constexpr (kVy) blk[kOffVy] = s.vy;
    }
    __device__ __forceinline__ void load(const RAYZ_CONSTANT R* g) { // g: the group's first word
        const RAYZ_CONSTANT pr* p = (const RAYZ_CONSTANT pr*)g;
#pragma unroll
        for (int q = 0; q < H; ++q) {
            cx[q] = p[kOffCx / 2 + q];
            if constexpr (kCy) cy[q] = p[kOffCy / 2 + q];
            if constexpr (kR2) cz[q] = p[kOffCz / 2 + q], r2[q] = p[kOffR2 / 2 + q];
            else cz[q] = p[kOffCz / 2 + q];
            if constexpr (kVy) vy[q] = p[kOffVy / 2 + q];
        }
    }
    __device__ __forceinline__ void ready(const RAYZ_CONSTANT R*& at) const {
        if constexpr (kVy) asm volatile("" : "+s"(at) : "s"(cx[0]), "s"(vy[0]));
        else asm volatile("" : "+s"(at) : "s"(cx[0]));
    }
    __device__ __forceinline__ void opaque() {
#pragma unroll
        for (int q = 0; q < H; ++q) {
            if constexpr (kR2) asm volatile("" : "+s"(cx[q]), "+s"(cz[q]), "+s"(r2[q]));
            else asm volatile("" : "+s"(cx[q]), "+s"(cz[q]));
            if constexpr (kCy) asm volatile("" : "+s"(cy[q]));
            if constexpr (kVy) asm volatile("" : "+s"(vy[q]));
        }
    }
    __device__ __forceinline__ void discs(R (&out)[G], const RayBasis<R>& b, [[maybe_unused]] R time) const {
        const R t2y = kVy ? time * b.e2y : R(0);
        [[maybe_unused]] const pr E1x{b.e1x, b.e1x}, E1z{b.e1z, b.e1z}, E2x{b.e2x, b.e2x}, E2y{b.e2y, b.e2y}, E2z{b.e2z, b.e2z},
            K1{b.k1, b.k1}, K2{b.k2, b.k2}, T2y{t2y, t2y}; // (a form uses E2y, T2y only with the field they multiply)
        pr p1[H], p2[H], d[H];
#pragma unroll
        for (int q = 0; q < H; ++q) p1[q] = __builtin_elementwise_fma(cx[q], E1x, K1);
#pragma unroll
        for (int q = 0; q < H; ++q) p2[q] = __builtin_elementwise_fma(cx[q], E2x, K2);
#pragma unroll
        for (int q = 0; q < H; ++q) p1[q] = __builtin_elementwise_fma(cz[q], E1z, p1[q]);
        if constexpr (kCy) {
#pragma unroll
            for (int q = 0; q < H; ++q) p2[q] = __builtin_elementwise_fma(cy[q], E2y, p2[q]);
        }
#pragma unroll
        for (int q = 0; q < H; ++q) p2[q] = __builtin_elementwise_fma(cz[q], E2z, p2[q]);
        if constexpr (kVy) {
#pragma unroll
            for (int q = 0; q < H; ++q) p2[q] = __builtin_elementwise_fma(vy[q], T2y, p2[q]);
        }
#pragma unroll
        for (int q = 0; q < H; ++q) d[q] = __builtin_elementwise_fma(-p2[q], p2[q], r2[q]);
#pragma unroll
        for (int q = 0; q < H; ++q) d[q] = __builtin_elementwise_fma(-p1[q], p1[q], d[q]);
#pragma unroll
        for (int q = 0; q < H; ++q) out[2 * q] = d[q].x, out[2 * q + 1] = d[q].y;
    }
    // The xy basis (kBasisXY): cy and vy enter p1 instead of cz.  Plane-run blocks (kCy = false) find the run's K1 in b.k1 as they
    // find K2 in b.k2.  Stage by stage across the group's pairs, as above.  R2all: the one padded r² of a form without the field.
    __device__ __forceinline__ void discs(R (&out)[G], const RayBasis<R, kBasisXY>& b, [[maybe_unused]] R time, [[maybe_unused]] R R2all = R(0)) const {
        const R t1y = kVy ? time * b.e1y : R(0), t2y = kVy ? time * b.e2y : R(0);
        [[maybe_unused]] const pr E1x{b.e1x, b.e1x}, E1y{b.e1y, b.e1y}, E2x{b.e2x, b.e2x}, E2y{b.e2y, b.e2y}, E2z{b.e2z, b.e2z},
            K1{b.k1, b.k1}, K2{b.k2, b.k2}, T1y{t1y, t1y}, T2y{t2y, t2y};
        pr p1[H], p2[H], d[H];
#pragma unroll
        for (int q = 0; q < H; ++q) p1[q] = __builtin_elementwise_fma(cx[q], E1x, K1);
#pragma unroll
        for (int q = 0; q < H; ++q) p2[q] = __builtin_elementwise_fma(cx[q], E2x, K2);
        if constexpr (kCy) {
#pragma unroll
            for (int q = 0; q < H; ++q) p1[q] = __builtin_elementwise_fma(cy[q], E1y, p1[q]);
#pragma unroll
            for (int q = 0; q < H; ++q) p2[q] = __builtin_elementwise_fma(cy[q], E2y, p2[q]);
        }
#pragma unroll
        for (int q = 0; q < H; ++q) p2[q] = __builtin_elementwise_fma(cz[q], E2z, p2[q]);
        if constexpr (kVy) {
#pragma unroll
            for (int q = 0; q < H; ++q) p1[q] = __builtin_elementwise_fma(vy[q], T1y, p1[q]);
#pragma unroll
            for (int q = 0; q < H; ++q) p2[q] = __builtin_elementwise_fma(vy[q], T2y, p2[q]);
        }
        if constexpr (kR2) {
#pragma unroll
            for (int q = 0; q < H; ++q) d[q] = __builtin_elementwise_fma(-p2[q], p2[q], r2[q]);
        } else {
            const pr RR{R2all, R2all};
#pragma unroll
            for (int q = 0; q < H; ++q) d[q] = __builtin_elementwise_fma(-p2[q], p2[q], RR);
        }
#pragma unroll
        for (int q = 0; q < H; ++q) d[q] = __builtin_elementwise_fma(-p1[q], p1[q], d[q]);
#pragma unroll
        for (int q = 0; q < H; ++q) out[2 * q] = d[q].x, out[2 * q + 1] = d[q].y;
    }
};
// The forms: their stream, and the slot their first block's first sphere has (DevScene's slot order).
template <class R> struct ScanGroup<R, 0> : PackedGroup<R, true, false> { // static
    template <class SC> static __device__ __forceinline__ const RAYZ_CONSTANT R* stream(const SC& sc) { return (const RAYZ_CONSTANT R*)sc.stat; }
    template <class SC> static __device__ __forceinline__ int slot0(const SC& sc) { return (int)plane_slots(sc.stat); }
};
template <class R> struct ScanGroup<R, 1> : PackedGroup<R, true, true> { // mov-Y
    template <class SC> static __device__ __forceinline__ const RAYZ_CONSTANT R* stream(const SC& sc) { return (const RAYZ_CONSTANT R*)sc.movy; }
    template <class SC> static __device__ __forceinline__ int slot0(const SC& sc) { return (int)(sc.ns_pad + plane_slots(sc.movy)); }
};
template <class R> struct ScanGroup<R, 3> : PackedGroup<R, false, false> { // static, plane run
    template <class SC> static __device__ __forceinline__ const RAYZ_CONSTANT R* stream(const SC& sc) { return (const RAYZ_CONSTANT R*)sc.stat; }
    template <class SC> static __device__ __forceinline__ int slot0(const SC&) { return 0; }
};
template <class R> struct ScanGroup<R, 4> : PackedGroup<R, false, true> { // mov-Y, plane run
    template <class SC> static __device__ __forceinline__ const RAYZ_CONSTANT R* stream(const SC& sc) { return (const RAYZ_CONSTANT R*)sc.movy; }
    template <class SC> static __device__ __forceinline__ int slot0(const SC& sc) { return (int)sc.ns_pad; }
};
// A speed bucket of a y-moving plane run: the static plane form (b.k2 = the bucket's K2) on the mov-Y class's slots.
template <class R> struct ScanGroup<R, 5> : ScanGroup<R, 3> {
    template <class SC> static __device__ __forceinline__ const RAYZ_CONSTANT R* stream(const SC& sc) { return (const RAYZ_CONSTANT R*)sc.movy; }
    template <class SC> static __device__ __forceinline__ int slot0(const SC& sc) { return (int)sc.ns_pad; }
};
// A one-radius set of a static run or of a speed bucket: cx and cz alone, in groups of kSetGroup (scan_sets is told its stream and slots).
template <class R> struct ScanGroup<R, 6> : PackedGroup<R, false, false, false, (int)rayz_plane::kSetGroup> {};
template <class R> struct ScanGroup<R, 2> { // mov-G
    typedef typename VecOf<R>::type r4;
    static constexpr int G = kMovGGroup;
    r4 c[G], v[G];
    template <class SC> static __device__ __forceinline__ const RAYZ_CONSTANT R* stream(const SC& sc) { return (const RAYZ_CONSTANT R*)sc.movg; }
    static constexpr int kWords = 8;
    __device__ __forceinline__ void load(const RAYZ_CONSTANT R* g) {
        const RAYZ_CONSTANT r4* p = (const RAYZ_CONSTANT r4*)g;
#pragma unroll
        for (int k = 0; k < G; ++k) c[k] = p[2 * k], v[k] = p[2 * k + 1];
    }
    __device__ __forceinline__ void ready(const RAYZ_CONSTANT R*& at) const { asm volatile("" : "+s"(at) : "s"(c[0].x)); }
    __device__ __forceinline__ void opaque() {
#pragma unroll
        for (int k = 0; k < G; ++k)
            asm volatile("" : "+s"(c[k].x), "+s"(c[k].y), "+s"(c[k].z), "+s"(c[k].w), "+s"(v[k].x), "+s"(v[k].y), "+s"(v[k].z));
    }
    __device__ __forceinline__ R disc(int k, const RayBasis<R>& b, R time) const {
        const R p1 = fm(v[k].z, time * b.e1z, fm(v[k].x, time * b.e1x, basis_p1<R>(b, c[k].x, c[k].z)));
        const R p2 = fm(v[k].z, time * b.e2z,
                        fm(v[k].y, time * b.e2y, fm(v[k].x, time * b.e2x, basis_p2<R>(b, c[k].x, c[k].y, c[k].z))));
        return basis_disc<R>(p1, p2, c[k].w);
    }
    __device__ __forceinline__ R disc(int k, const RayBasis<R, kBasisXY>& b, R time) const { // (p1 has y where the form above has z)
        const R p1 = fm(v[k].y, time * b.e1y, fm(v[k].x, time * b.e1x, fm(c[k].y, b.e1y, fm(c[k].x, b.e1x, b.k1))));
        const R p2 = fm(v[k].z, time * b.e2z,
                        fm(v[k].y, time * b.e2y, fm(v[k].x, time * b.e2x, fm(c[k].z, b.e2z, fm(c[k].y, b.e2y, fm(c[k].x, b.e2x, b.k2))))));
        return basis_disc<R>(p1, p2, c[k].w);
    }
    template <int AX> __device__ __forceinline__ void discs(R (&out)[G], const RayBasis<R, AX>& b, R time) const {
#pragma unroll
        for (int k = 0; k < G; ++k) out[k] = disc(k, b, time);
    }
    template <class SC> static __device__ __forceinline__ int slot0(const SC& sc) { return (int)(sc.ns_pad + sc.ny_pad); }
};

// What the scan needs of one ray (one of the NR rays a lane carries).
template <class R, int AX = kBasisXZ> struct ScanRay {
    V<R> o, d;
    R time;
    RayBasis<float, AX> basis; // the reject test runs in f32 for both precisions (FilterR): built from ud, o narrowed to f32
    float ftime;
    double inv_a2; // 1 / (d·d) in f64, for the narrow phase
    R tbest;
    int ibest;
    uint32_t cand[4]; // parked candidate slots (spheres whose line-distance test passed), evaluated by narrow_flush
    uint32_t ncand;
};

// Reject tests of one group for the lane's NR rays; the running maximum feeds the pair's single branch.
template <class R, int CLS, int NR, int AX>
__device__ __forceinline__ void group_discs(const ScanGroup<float, CLS>& g, ScanRay<R, AX> (&ray)[NR],
                                            float (&disc)[NR][ScanGroup<float, CLS>::G], float& m, bool first) {
    constexpr int G = ScanGroup<float, CLS>::G;
#pragma unroll
    for (int r = 0; r < NR; ++r) {
        g.discs(disc[r], ray[r].basis, ray[r].ftime);
#pragma unroll
        for (int k = 0; k < G; ++k) m = (first && r == 0 && k == 0) ? disc[0][0] : mx(m, disc[r][k]);
    }
}
// Evaluate every parked candidate of the wave's lanes (round j: lanes with more than j parked slots).
template <class R, int NR, int AX> __device__ __forceinline__ void narrow_flush(const DevScene<R>& sc, ScanRay<R, AX> (&ray)[NR], R tmin) {
#pragma unroll
    for (int r = 0; r < NR; ++r) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (__ballot(ray[r].ncand > (uint32_t)j) == 0ull) break;
            if (ray[r].ncand > (uint32_t)j) {
                const uint32_t slot = ray[r].cand[j];
                narrow_eval<R>(sc.slot64[2 * slot], sc.slot64[2 * slot + 1], (int)sc.slot_pool[slot], ray[r].o, ray[r].d,
                               ray[r].time, ray[r].inv_a2, tmin, ray[r].tbest, ray[r].ibest);
            }
        }
        ray[r].ncand = 0;
    }
}
// Park one group's candidates (slots first .. first+G-1); a lane whose list is full forces a flush first.
template <class R, int CLS, int NR, int AX>
__device__ __forceinline__ void group_collect(const DevScene<R>& sc, int first, ScanRay<R, AX> (&ray)[NR],
                                              const float (&disc)[NR][ScanGroup<float, CLS>::G], R tmin) {
    constexpr int G = ScanGroup<float, CLS>::G;
#pragma unroll
    for (int k = 0; k < G; ++k)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            const bool want = disc[r][k] >= 0.0f;
            // usually ONE of the group's spheres made the wave take this path: the others cost a compare and a scalar
            // branch instead of the whole insertion (a small scene takes this path in almost every group: measured +2.5 %
            // on config 2; parking whole group pairs in LDS and re-testing them per lane afterwards was 13 % SLOWER)
            if (__ballot(want) == 0ull) continue;
            if (__ballot(want && ray[r].ncand == 4u) != 0ull) narrow_flush<R, NR>(sc, ray, tmin);
            if (want) {
                const uint32_t slot = (uint32_t)(first + k), n = ray[r].ncand;
                ray[r].cand[0] = n == 0u ? slot : ray[r].cand[0];
                ray[r].cand[1] = n == 1u ? slot : ray[r].cand[1];
                ray[r].cand[2] = n == 2u ? slot : ray[r].cand[2];
                ray[r].cand[3] = n == 3u ? slot : ray[r].cand[3];
                ray[r].ncand = n + 1u;
            }
        }
}

// One velocity class.  n is a multiple of 2·G and the stream carries two spare groups.  Scalar loads return out of order,
// so a wave can only wait for all of them (lgkmcnt(0)): every load is therefore issued right AFTER a wait, into the set
// that is free, and has the 12 – 16 packed FMAs of the other set's test in front of the wait that covers it.  Per iteration:
// wait for a, load b with the next group, test a; wait for b, load a with the group after it, test b; then ONE reject
// branch for the 2·G tests (≈10 cycles of a wave's time: once per 8 tests, not 4), wave-uniform by a ballot.  (The
// sched_barriers keep hipcc from moving the tests across the waits.)  The loop carries the stream pointer `at` of the
// group pair (the loads' offsets from it are immediates) and a down-counter of the slots left, from which the candidate
// branch, the only user of the slot number, recovers it.  The furthest group a scan loads is the one behind its last pair:
// rayz_plane::scan_reach, held inside every section's spare groups where the host builds the streams.
// scan_blocks tests the stream's slots i0 .. i1 (relative to the class's first slot, ScanGroup::slot0).
template <class R, int CLS, int NR, int AX>
__device__ __forceinline__ void scan_blocks(const DevScene<R>& sc, const RAYZ_CONSTANT float* base, int i0, int i1,
                                            ScanRay<R, AX> (&ray)[NR], R tmin) {
    typedef ScanGroup<float, CLS> Grp;
    constexpr int G = Grp::G, W = Grp::kWords * G; // words of a group
    const RAYZ_CONSTANT float* at = base + Grp::kWords * i0;
    Grp a, b;
    a.load(at);
#ifdef RAYZ_DEBUG_NOFEED
    b.load(at + W);
#endif
    for (int left = i1 - i0; left > 0; left -= 2 * G, at += 2 * W) {
        float da[NR][G], db[NR][G];
        float m = -1.0f;
#ifdef RAYZ_DEBUG_NOFEED // timing experiment only: never reload (wrong results); values kept opaque to the compiler
        a.opaque();
        group_discs<R, CLS, NR>(a, ray, da, m, true);
        b.opaque();
        group_discs<R, CLS, NR>(b, ray, db, m, false);
#else
        a.ready(at);
        b.load(at + W);
        __builtin_amdgcn_sched_barrier(0);
        group_discs<R, CLS, NR>(a, ray, da, m, true);
        __builtin_amdgcn_sched_barrier(0);
        b.ready(at);
        a.load(at + 2 * W);
        __builtin_amdgcn_sched_barrier(0);
        group_discs<R, CLS, NR>(b, ray, db, m, false);
#endif
#ifdef RAYZ_DEBUG_NONARROW // timing experiment only (wrong results)
        if (__ballot(m >= 1e30f) != 0ull) {
#else
        if (__ballot(m >= 0.0f) != 0ull) { // any lane, any ray, any of the 2·G spheres: rare.  Lanes that have none park nothing
#endif
            const int first = Grp::slot0(sc) + i1 - left;
            group_collect<R, CLS, NR>(sc, first, ray, da, tmin);
            group_collect<R, CLS, NR>(sc, first + G, ray, db, tmin);
        }
    }
}
template <class R, int CLS, int NR, int AX>
__device__ __forceinline__ void scan_class(const DevScene<R>& sc, int n, ScanRay<R, AX> (&ray)[NR], R tmin) {
    if (n == 0) return;
    // the stream's base as a value of its own: read out of the kernel arguments it is one lane of a 16-register block,
    // and a spilled block comes back whole (the f64 kernel paid 20 v_readlane per iteration for this one pointer)
    const RAYZ_CONSTANT float* base = ScanGroup<float, CLS>::stream(sc);
    if constexpr (sizeof(R) == 8) asm volatile("" : "+s"(base));
    scan_blocks<R, CLS, NR>(sc, base, 0, n, ray, tmin);
}
// The one-radius sets' loop (xy basis only): scan_blocks' order of waits, loads and tests over two-field groups of kSetGroup = 8,
// each ONE 16-word scalar load into 16 SGPRs (two sets: 32, where the three-field form of 4 holds 24), with the set's padded r²
// as the loop-invariant operand R2 and one reject decision per 16 tests.  `slot0`: the class's first slot.
template <class R, int NR>
__device__ __forceinline__ void scan_sets(const DevScene<R>& sc, const RAYZ_CONSTANT float* base, int i0, int i1, int slot0,
                                          ScanRay<R, kBasisXY> (&ray)[NR], R tmin, float R2) {
    typedef ScanGroup<float, 6> Grp;
    constexpr int G = Grp::G, W = Grp::kWords * G;
    const RAYZ_CONSTANT float* at = base + Grp::kWords * i0;
    Grp a, b;
    a.load(at);
    for (int left = i1 - i0; left > 0; left -= 2 * G, at += 2 * W) {
        float da[NR][G], db[NR][G];
        float m = -1.0f;
        a.ready(at);
        b.load(at + W);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            a.discs(da[r], ray[r].basis, ray[r].ftime, R2);
#pragma unroll
            for (int k = 0; k < G; ++k) m = (r == 0 && k == 0) ? da[0][0] : mx(m, da[r][k]);
        }
        __builtin_amdgcn_sched_barrier(0);
        b.ready(at);
        a.load(at + 2 * W);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            b.discs(db[r], ray[r].basis, ray[r].ftime, R2);
#pragma unroll
            for (int k = 0; k < G; ++k) m = mx(m, db[r][k]);
        }
        if (__ballot(m >= 0.0f) != 0ull) {
            const int first = slot0 + i1 - left;
            group_collect<R, 6, NR>(sc, first, ray, da, tmin);
            group_collect<R, 6, NR>(sc, first + G, ray, db, tmin);
        }
    }
}
// A plane run's K2 for one ray: cy·e2y + k2 in ONE rounding (the run loop below and RAYZ_KAT_SCAN_DISCS classes 2 / 3).
__device__ __forceinline__ float plane_run_k2(float cy, float e2y, float k2) { return fm(cy, e2y, k2); }
// A speed bucket's K2 for one ray: the run's K2, then v0·(time·e2y) in one more rounding (the bucket loop below and
// RAYZ_KAT_SCAN_DISCS class 4).
__device__ __forceinline__ float bucket_k2(float v0, float cy, float ftime, float e2y, float k2) {
    return fm(v0, ftime * e2y, plane_run_k2(cy, e2y, k2));
}
// The xy basis (kBasisXY): e1 has a y component, and a run's or bucket's K1 is made of (e1y, k1) as its K2 is of (e2y, k2).
__device__ __forceinline__ float plane_run_k1(float cy, float e1y, float k1) { return plane_run_k2(cy, e1y, k1); }
__device__ __forceinline__ float bucket_k1(float v0, float cy, float ftime, float e1y, float k1) { return bucket_k2(v0, cy, ftime, e1y, k1); }
// The xy basis's own k1 of a ray whose basis holds a run's K1 in its place: made again from the origin (two FMAs per ray and run;
// a saved copy is one more register alive through the scan loops, and cost the f32 kernel two spilled VGPRs), bit for bit what
// scan_begin's make_basis made: the same function of the same narrowed origin.
template <class R> __device__ __forceinline__ float scan_k1(const ScanRay<R, kBasisXY>& ray) {
    return basis_xy_k1<float>(ray.basis, (float)ray.o.x, (float)ray.o.y);
}
// The static (CLS 0) or mov-Y (CLS 1) class: its plane runs, then its loose spheres.  Per run, K2 = fm(cy, e2y, k2) replaces
// each ray's k2 (one FMA per ray and run), which is put back before the loose spheres.  The head is read here, every scan
// (the empty asm keeps the compiler from loading it once per kernel and holding it in spilled SGPRs).
// kSets (flat_one_radius_kernel): the stream's set section (behind everything else; found from what the head and the bucket table
// say of the stream's length, rayz_hip.hip: append_sets) names the one-radius sets, tested last by scan_sets, and the first slot the
// old forms still test of each run and bucket.
template <class R, int CLS, int NR, int AX, bool kSets = false>
__device__ __forceinline__ void scan_plane_class(const DevScene<R>& sc, int n_class, ScanRay<R, AX> (&ray)[NR], R tmin) {
    constexpr int P = ScanGroup<float, CLS + 3>::kWords, G = ScanGroup<float, CLS>::G; // words per plane sphere: the run form's
    const RAYZ_CONSTANT float* head = ScanGroup<float, CLS>::stream(sc);
    asm volatile("" : "+s"(head));
    const RAYZ_CONSTANT uint32_t* h = (const RAYZ_CONSTANT uint32_t*)head;
    const int nr = (int)h[0], plane = (int)h[1];
    [[maybe_unused]] const RAYZ_CONSTANT uint32_t* sh = h; // the set section's header
    if constexpr (kSets) {
        uint32_t end = (uint32_t)(kPlaneHeader + P * (plane + 2 * G) + ScanGroup<float, CLS>::kWords * (n_class - plane + 2 * G));
        if constexpr (CLS == 1) {
            const uint32_t nb = h[3];
            const RAYZ_CONSTANT SpeedBucket* bk = (const RAYZ_CONSTANT SpeedBucket*)(head + h[2] + kBucketHeader);
            end = h[2] + kBucketHeader;
            if (nb != 0u) end = bk[nb - 1u].base + ScanGroup<float, 5>::kWords * bk[nb - 1u].end;
            end += ScanGroup<float, 5>::kWords * 2 * G;
        }
        sh = h + rayz_plane::set_section(end);
    }
    if (nr != 0) {
        const RAYZ_CONSTANT PlaneRun* runs = (const RAYZ_CONSTANT PlaneRun*)(h + 4);
        float k2[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) k2[r] = ray[r].basis.k2;
        for (int j = 0; j < nr; ++j) {
            const float cy = runs[j].cy;
            int first = (int)runs[j].first;
            const int end = (int)runs[j].end;
            if constexpr (kSets) { // .. or to its one-radius sets
                first = (int)sh[4 + j];
                if (first == end) continue;
            } else if constexpr (CLS == 1) { // the run's first slots belong to its speed buckets (below)
                first = (int)((const RAYZ_CONSTANT uint32_t*)(head + h[2]))[j];
                if (first == end) continue;
            }
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                ray[r].basis.k2 = plane_run_k2(cy, ray[r].basis.e2y, k2[r]);
                if constexpr (AX == kBasisXY) ray[r].basis.k1 = plane_run_k1(cy, ray[r].basis.e1y, scan_k1(ray[r]));
            }
            scan_blocks<R, CLS + 3, NR>(sc, head + kPlaneHeader, first, end, ray, tmin);
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            ray[r].basis.k2 = k2[r];
            if constexpr (AX == kBasisXY) ray[r].basis.k1 = scan_k1(ray[r]);
        }
    }
    if (n_class > plane) scan_blocks<R, CLS, NR>(sc, head + kPlaneHeader + P * (plane + 2 * G), 0, n_class - plane, ray, tmin);
    if constexpr (CLS == 1) { // the speed buckets, after the loose spheres (scan order is free: scan_sphere_classes)
        const int nb = (int)h[3];
        if (nb != 0) {
            const RAYZ_CONSTANT SpeedBucket* bk = (const RAYZ_CONSTANT SpeedBucket*)(head + h[2] + kBucketHeader);
            if constexpr (kSets) bk = (const RAYZ_CONSTANT SpeedBucket*)(sh + rayz_plane::kSetHeader + 8u * sh[0]); // (first: behind the bucket's sets)
            float k2[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) k2[r] = ray[r].basis.k2;
            for (int j = 0; j < nb; ++j) {
                const float v0 = bk[j].v0, cy = bk[j].cy;
                if constexpr (kSets)
                    if (bk[j].first == bk[j].end) continue;
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    ray[r].basis.k2 = bucket_k2(v0, cy, ray[r].ftime, ray[r].basis.e2y, k2[r]);
                    if constexpr (AX == kBasisXY) ray[r].basis.k1 = bucket_k1(v0, cy, ray[r].ftime, ray[r].basis.e1y, scan_k1(ray[r]));
                }
                scan_blocks<R, 5, NR>(sc, head + bk[j].base, (int)bk[j].first, (int)bk[j].end, ray, tmin);
            }
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                ray[r].basis.k2 = k2[r];
                if constexpr (AX == kBasisXY) ray[r].basis.k1 = scan_k1(ray[r]);
            }
        }
    }
    if constexpr (kSets) {
        static_assert(AX == kBasisXY && sizeof(rayz_plane::RadiusSet) == 32, "the sets are scanned in the xy basis");
        const int ns = (int)sh[0];
        if (ns != 0) {
            const RAYZ_CONSTANT rayz_plane::RadiusSet* st = (const RAYZ_CONSTANT rayz_plane::RadiusSet*)(sh + rayz_plane::kSetHeader);
            float k2[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) k2[r] = ray[r].basis.k2;
            for (int j = 0; j < ns; ++j) {
                const float v0 = st[j].v0, cy = st[j].cy;
#pragma unroll
                for (int r = 0; r < NR; ++r) { // a static run's K1, K2, or its bucket's: the very values the old form tests it with
                    ray[r].basis.k2 = CLS == 1 ? bucket_k2(v0, cy, ray[r].ftime, ray[r].basis.e2y, k2[r]) : plane_run_k2(cy, ray[r].basis.e2y, k2[r]);
                    ray[r].basis.k1 = CLS == 1 ? bucket_k1(v0, cy, ray[r].ftime, ray[r].basis.e1y, scan_k1(ray[r])) : plane_run_k1(cy, ray[r].basis.e1y, scan_k1(ray[r]));
                }
                scan_sets<R, NR>(sc, head + st[j].base, (int)st[j].first, (int)st[j].end, ScanGroup<float, CLS + 3>::slot0(sc), ray, tmin, st[j].R2);
            }
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                ray[r].basis.k2 = k2[r];
                ray[r].basis.k1 = scan_k1(ray[r]);
            }
        }
    }
}
// Every sphere class in slot order (the slot order only matters to the candidates' parking order; the acceptance rule
// decides ties by pool index, so the hit is the same in any order).
template <class R, int NR, bool kSets = false, int AX> __device__ __forceinline__ void scan_sphere_classes(const DevScene<R>& sc, ScanRay<R, AX> (&ray)[NR], R tmin) {
    scan_plane_class<R, 0, NR, AX, kSets>(sc, (int)sc.ns_pad, ray, tmin);
    scan_plane_class<R, 1, NR, AX, kSets>(sc, (int)sc.ny_pad, ray, tmin);
    scan_class<R, 2, NR>(sc, (int)sc.ng_pad, ray, tmin);
}

// Triangle stream of the flat list: same ping-pong scalar prefetch, groups of kTriGroup.
template <class R> struct TriGroup {
    typedef typename VecOf<R>::type r4;
    r4 a[kTriGroup], b[kTriGroup], c[kTriGroup];
    __device__ __forceinline__ void load(const RAYZ_CONSTANT R* base, int i) {
        const RAYZ_CONSTANT r4* p = (const RAYZ_CONSTANT r4*)base + 3 * i;
#pragma unroll
        for (int k = 0; k < kTriGroup; ++k) a[k] = p[3 * k], b[k] = p[3 * k + 1], c[k] = p[3 * k + 2];
    }
    __device__ __forceinline__ void touch() const { asm volatile("" ::"s"(a[0].x)); }
    template <int NR, int AX>
    __device__ __forceinline__ void test(const DevScene<R>& sc, int i, ScanRay<R, AX> (&ray)[NR], R tmin) const {
        R f[NR][kTriGroup];
        R m = R(-1);
#pragma unroll
        for (int r = 0; r < NR; ++r)
#pragma unroll
            for (int k = 0; k < kTriGroup; ++k) {
                f[r][k] = tri_filter<R>(V<R>{a[k].x, a[k].y, a[k].z}, V<R>{b[k].x, b[k].y, b[k].z},
                                        V<R>{c[k].x, c[k].y, c[k].z}, ray[r].o, ray[r].d);
                m = (r == 0 && k == 0) ? f[0][0] : mx(m, f[r][k]);
            }
        if (m >= R(0)) {
#pragma unroll
            for (int k = 0; k < kTriGroup; ++k)
#pragma unroll
                for (int r = 0; r < NR; ++r)
                    tri_accept<R>(f[r][k], V<R>{a[k].x, a[k].y, a[k].z}, V<R>{b[k].x, b[k].y, b[k].z},
                                  V<R>{c[k].x, c[k].y, c[k].z}, ray[r].o, ray[r].d, tmin, (int)sc.n_spheres + i + k,
                                  ray[r].tbest, ray[r].ibest);
        }
    }
};
template <class R, int NR, int AX>
__device__ __forceinline__ void scan_triangles(const DevScene<R>& sc, ScanRay<R, AX> (&ray)[NR], R tmin) {
    const int n = (int)sc.nt_pad;
    if (n == 0) return;
    const RAYZ_CONSTANT R* base = (const RAYZ_CONSTANT R*)sc.tri;
    if constexpr (sizeof(R) == 8) asm volatile("" : "+s"(base));
    TriGroup<R> a, b;
    a.load(base, 0);
    for (int i = 0; i < n; i += 2 * kTriGroup) {
        a.touch();
        b.load(base, i + kTriGroup);
        __builtin_amdgcn_sched_barrier(0);
        a.template test<NR>(sc, i, ray, tmin);
        b.touch();
        a.load(base, i + 2 * kTriGroup);
        __builtin_amdgcn_sched_barrier(0);
        b.template test<NR>(sc, i + kTriGroup, ray, tmin);
    }
}

// ---- the flat-list scan: nearest hit of each of the lane's NR rays over every hittable -------------------
// Wave-uniform in the sphere index: records arrive by scalar loads and feed the VALU as SGPR operands.  What
// bounds the loop was established by elimination (tools/ubench/): not the sphere feed (a build
// that never reloads ran in the same time in round 2; 4 % per segment in round 7, half of which scan_blocks' order of loads
// and discs' order of FMAs recovered), not occupancy, not instruction-level parallelism — but the rate at
// which VALU instructions can read DIFFERENT scalar registers (≈2.75 cycles each), plus ≈10 cycles per reject
// branch.  Hence two spheres per packed FMA (ScanGroup::discs) and one branch per 8 tests (scan_class).
// NR = rays per lane; the product instantiates NR = 1 (two rays per lane halve the scalar loads per test and
// were measured no faster).
template <class R, int NR, int AX>
__device__ __forceinline__ void scan_begin(ScanRay<R, AX>& ray, V<R> o, V<R> d, V<R> ud, R time) {
    ray.o = o;
    ray.d = d;
    ray.time = time;
    ray.basis = make_basis<float, AX>(V<float>{(float)ud.x, (float)ud.y, (float)ud.z}, V<float>{(float)o.x, (float)o.y, (float)o.z});
    ray.ftime = (float)time;
    const double ddx = d.x, ddy = d.y, ddz = d.z;
    ray.inv_a2 = 1.0 / fm(ddz, ddz, fm(ddy, ddy, ddx * ddx));
    ray.tbest = (R)__builtin_inff();
    ray.ibest = -1;
    ray.cand[0] = ray.cand[1] = ray.cand[2] = ray.cand[3] = 0u;
    ray.ncand = 0u;
}
template <class R, int NR, bool kSets = false, int AX> __device__ __forceinline__ void scan_spheres(const DevScene<R>& sc, ScanRay<R, AX> (&ray)[NR], R tmin) {
    scan_sphere_classes<R, NR, kSets>(sc, ray, tmin);
    narrow_flush<R, NR>(sc, ray, tmin);
    scan_triangles<R, NR>(sc, ray, tmin);
}

} // namespace rayz_dev
