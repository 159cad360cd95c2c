// known_answers_kernel.hpp — the known-answer entry's kernel (rayz_hip_kat): the render path's own device functions evaluated on
// caller-supplied records, one operation per `op`.  The host side is known_answers.hpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bvh_walk.hpp"
#include "device_math.hpp"
#include "device_types.hpp"
#include "flat_scan.hpp"
#include "shade.hpp"

namespace rayz_dev {

// ---- known-answer entry (rayz_hip_kat): the kernel's own device functions on caller-supplied inputs -----------------
// One thread per record; records are RAYZ_KAT_IN_STRIDE doubles in, RAYZ_KAT_OUT_STRIDE doubles out (layouts in
// include/rayz_hip.h).  Inputs are narrowed to R exactly as the scene and camera are when they cross the ABI.
constexpr int kKatIn = 48, kKatOut = 12;
// One block of the scan in form CLS from a known-answer record (cx[4] at 0, cy[4] at 4, cz[4] at 8, vy[4] at 16, padded r²[4]
// at 28: the form takes the fields it has), through ScanGroup::discs as the scan loop runs it.
template <int CLS, int AX> __device__ __forceinline__ void kat_block_discs(const double* a, const RayBasis<float, AX>& b, float ft, float (&out)[4]) {
    ScanGroup<float, CLS> g;
    auto pair = [&](int at, int q) { return f2{(float)a[at + 2 * q], (float)a[at + 2 * q + 1]}; };
    for (int q = 0; q < 2; ++q) g.cx[q] = pair(0, q), g.cy[q] = pair(4, q), g.cz[q] = pair(8, q), g.vy[q] = pair(16, q), g.r2[q] = pair(28, q);
    g.discs(out, b, ft);
}
template <class R> __global__ __launch_bounds__(64) void kat_kernel(uint32_t op, const double* in, uint32_t n, double* out) {
    typedef typename VecOf<R>::type r4;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* a = in + (size_t)i * kKatIn;
    double* r = out + (size_t)i * kKatOut;
    for (int k = 0; k < kKatOut; ++k) r[k] = 0.0;
    auto v3 = [&](int k) { return V<R>{(R)a[k], (R)a[k + 1], (R)a[k + 2]}; };
    auto put3 = [&](int k, V<R> v) { r[k] = (double)v.x, r[k + 1] = (double)v.y, r[k + 2] = (double)v.z; };
    switch (op) {
    case 0: { // REFRACT: ud(3) n(3) eta -> dir(3)
        const V<R> ud = v3(0), nrm = v3(3);
        put3(0, refract<R>(ud, nrm, -dot3(ud, nrm), (R)a[6]));
        break;
    }
    case 1: // REFLECTANCE: cos, eta -> r
        r[0] = (double)reflectance<R>((R)a[0], (R)a[1]);
        break;
    case 2: { // GET_RAY: from du dv pxo defu defv (18) defocus px py n_u u[..] -> origin(3) dir(3) time draws
        DevCamera<R> cam;
        for (int k = 0; k < 3; ++k) {
            cam.from[k] = (R)a[k], cam.du[k] = (R)a[3 + k], cam.dv[k] = (R)a[6 + k], cam.pxo[k] = (R)a[9 + k];
            cam.defu[k] = (R)a[12 + k], cam.defv[k] = (R)a[15 + k];
        }
        cam.defocus = a[18] != 0.0 ? 1u : 0u;
        cam._pad = 0;
        ListRng g{a + 22, a[21] < 0.0 ? 0u : (uint32_t)a[21], 0u};
        V<R> o, d;
        R time;
        if (a[21] < 0.0) camera_ray_no_rng<R>(cam, (uint32_t)a[19], (uint32_t)a[20], o, d, time); // n_u = -1: getRay(px, py, null)
        else camera_ray<R>(cam, g, (uint32_t)a[19], (uint32_t)a[20], o, d, time);
        put3(0, o);
        put3(3, d);
        r[6] = (double)time;
        r[7] = (double)g.i;
        break;
    }
    case 3: { // BOX_HIT: lo(3) hi(3) o(3) d(3) tmin tmax ... format[26] -> hit, t_entry.  The box as the device holds it, in
              // either record format (DevScene::bvh_nodes), made by the host from the record as the scene upload makes it
              // (rayz_hip_kat): format 0: a[14..19] = 16-bit plane indices lo.xyz hi.xyz, a[20..25] = grid origin and cell size;
              // format 1: a[14..19] = the padded planes rounded outward to f32, the grid = origin 0, cell 1
        DevScene<R> g{};
        for (int k = 0; k < 3; ++k) g.bvh_glo[k] = (float)a[20 + k], g.bvh_cell[k] = (float)a[23 + k];
        BvhQuery<R> q;
        const V<R> d = v3(9);
        bvh_begin<R>(q, g, v3(6), d, unit(d), 1u);
        q.tbest = (R)a[13];
        q.tb32 = round_up_f32(q.tbest);
        float t0;
        if (a[26] != 0.0) {
            r[0] = bvh_box_hit_planes<R, false>(V<float>{(float)a[14], (float)a[15], (float)a[16]}, V<float>{(float)a[17], (float)a[18], (float)a[19]},
                                                q, round_down_f32((R)a[12]), t0) ? 1.0 : 0.0;
        } else {
            const uint32_t wx = (uint32_t)a[14] | ((uint32_t)a[17] << 16), wy = (uint32_t)a[15] | ((uint32_t)a[18] << 16),
                           wz = (uint32_t)a[16] | ((uint32_t)a[19] << 16);
            r[0] = bvh_box_hit<R>(wx, wy, wz, q, round_down_f32((R)a[12]), t0) ? 1.0 : 0.0;
        }
        r[1] = (double)t0;
        break;
    }
    case 4: { // SPHERE_HIT: c(3) v(3) radius o(3) d(3) time tmin tmax -> hit t point(3) normal(3) front filter
        const V<R> o = v3(7), d = v3(10);
        const R time = (R)a[13], tmin = (R)a[14];
        const r4 c = {(R)a[0], (R)a[1], (R)a[2], (R)a[16]}, v = {(R)a[3], (R)a[4], (R)a[5], R(0)}; // a[16]: padded r² (f32), from the host
        const V<R> ud = unit(d);
        // the reject test as the kernels run it: f32 for both precisions, the ray narrowed to f32
        const RayBasis<float> b = make_basis<float>(V<float>{(float)ud.x, (float)ud.y, (float)ud.z}, V<float>{(float)o.x, (float)o.y, (float)o.z});
        const bool cand = leaf_reject_test(b, (float)time, V<float>{(float)c.x, (float)c.y, (float)c.z},
                                           V<float>{(float)v.x, (float)v.y, (float)v.z}, (float)c.w);
        r[9] = cand ? 1.0 : 0.0;
        R tbest = (R)a[15];
        int ibest = -1;
        if (cand) {
            const double ddx = d.x, ddy = d.y, ddz = d.z;
            const double inv_a2 = 1.0 / fm(ddz, ddz, fm(ddy, ddy, ddx * ddx));
            const d4 c64 = {a[0], a[1], a[2], a[6] * a[6]}, v64 = {a[3], a[4], a[5], 0.0};
            // the reference accepts t <= tmax (src/geom.zig:56-58); the kernel's running best is exclusive with a tie
            // rule on the pool index: index 1 > the initial -1 makes a tie with tmax an accept here too
            narrow_eval<R>(c64, v64, 1, o, d, time, inv_a2, tmin, tbest, ibest);
        }
        if (ibest >= 0) {
            V<R> pt, nrm;
            sphere_hit_record<R>(c, v, o, d, time, tbest, pt, nrm);
            const bool front = face_forward<R>(d, nrm);
            r[0] = 1.0, r[1] = (double)tbest;
            put3(2, pt);
            put3(5, nrm);
            r[8] = front ? 1.0 : 0.0;
        }
        break;
    }
    case 5: { // SCATTER: kind method param o(3) d(3) point(3) normal(3) front n_u u[..] -> ok dir(3) draws
        const uint32_t kind = (uint32_t)a[0], method = (uint32_t)a[1];
        const R param = (R)a[2];
        const V<R> d = v3(6);
        ListRng g{a + 17, (uint32_t)a[16], 0u};
        V<R> nd{R(0), R(0), R(0)};
        const bool ok = scatter_dir<R>(kind, method, param, R(1) / param, g, d, unit(d), v3(9), v3(12), a[15] != 0.0, nd);
        r[0] = ok ? 1.0 : 0.0;
        put3(1, nd);
        r[4] = (double)g.i;
        break;
    }
    case 6: // CHECKER: p(3) scale -> parity
        r[0] = (double)checker_parity<R>(v3(0), (R)a[3]);
        break;
    case 7: { // BACKGROUND: d(3) -> colour(3)
        put3(0, background<R>(unit(v3(0))));
        break;
    }
    case 8: { // TRIANGLE_HIT (build-defined): v0(3) v1(3) v2(3) o(3) d(3) tmin tmax -> hit t filter>=0
        const V<R> v0 = v3(0), o = v3(9), d = v3(12);
        const V<R> e1{(R)(a[3] - a[0]), (R)(a[4] - a[1]), (R)(a[5] - a[2])}, e2{(R)(a[6] - a[0]), (R)(a[7] - a[1]), (R)(a[8] - a[2])};
        const R f = tri_filter<R>(v0, e1, e2, o, d);
        R tbest = (R)a[16];
        int ibest = -1;
        tri_accept<R>(f, v0, e1, e2, o, d, (R)a[15], 1, tbest, ibest);
        r[0] = ibest >= 0 ? 1.0 : 0.0;
        r[1] = ibest >= 0 ? (double)tbest : 0.0;
        r[2] = f >= R(0) ? 1.0 : 0.0;
        break;
    }
    case 9: { // SCAN_DISCS: one block of the flat list's scan, THROUGH the packed-FMA form the scan loop runs
              // (ScanGroup<float, CLS>::discs: two spheres per v_pk_fma_f32), plus the general-velocity form of the BVH
              // leaves on the same spheres: cx[4] cy[4] cz[4] radius[4] vy[4] o(3) d(3) time cls (+ padded r²[4] at 28, from the
              // host) want_r2 -> disc[4] leaf_disc[4] r²[4] (if want_r2, else 0).  cls (checked by the host): 0 static, 1 mov-Y (the loose forms), 2 static,
              // 3 mov-Y plane run (the run forms, cy[4] the run's height, K2 put in the basis as scan_plane_class does)
        const V<R> o = v3(20), d = v3(23);
        const V<R> ud = unit(d);
        const RayBasis<float> b = make_basis<float>(V<float>{(float)ud.x, (float)ud.y, (float)ud.z}, V<float>{(float)o.x, (float)o.y, (float)o.z});
        const float ft = (float)(R)a[26];
        const int cls = (int)a[27];
        const bool movy = cls == 1 || cls == 3;
        RayBasis<float> bk = b;
        if (cls >= 2) bk.k2 = plane_run_k2((float)a[4], b.e2y, b.k2);
        float out4[4];
        if (cls == 0) kat_block_discs<0>(a, bk, ft, out4);
        else if (cls == 1) kat_block_discs<1>(a, bk, ft, out4);
        else if (cls == 2) kat_block_discs<3>(a, bk, ft, out4);
        else kat_block_discs<4>(a, bk, ft, out4);
        for (int k = 0; k < 4; ++k) {
            r[k] = (double)out4[k];
            const float vy = movy ? (float)a[16 + k] : 0.0f;
            const float p1 = fm(0.0f, ft * b.e1z, fm(0.0f, ft * b.e1x, basis_p1<float>(b, (float)a[k], (float)a[8 + k])));
            const float p2 = fm(0.0f, ft * b.e2z, fm(vy, ft * b.e2y, fm(0.0f, ft * b.e2x, basis_p2<float>(b, (float)a[k], (float)a[4 + k], (float)a[8 + k]))));
            r[4 + k] = (double)basis_disc<float>(p1, p2, (float)a[28 + k]);
            r[8 + k] = a[32] != 0.0 ? (double)(float)a[28 + k] : 0.0;
        }
        break;
    }
    case 10: { // BUCKET_DISCS: one block of a speed bucket (scan_plane_class's bucket loop): cx[4] cy[0] cz[4] radius[4] vy[4]
               // o(3) d(3) time v0 (+ the bucket's padded r2b[4] at 28, from the host) -> disc[4] K2b 0 0 0 r2b[4]
        const V<R> o = v3(20), d = v3(23);
        const V<R> ud = unit(d);
        RayBasis<float> b = make_basis<float>(V<float>{(float)ud.x, (float)ud.y, (float)ud.z}, V<float>{(float)o.x, (float)o.y, (float)o.z});
        b.k2 = bucket_k2((float)a[27], (float)a[4], (float)(R)a[26], b.e2y, b.k2);
        float out4[4];
        kat_block_discs<5>(a, b, 0.0f, out4);
        for (int k = 0; k < 4; ++k) r[k] = (double)out4[k], r[8 + k] = (double)(float)a[28 + k];
        r[4] = (double)b.k2;
        break;
    }
    case 11: { // SCAN_DISCS_XY: SCAN_DISCS' record through the xy basis (kBasisXY, flat_xy_kernel's): the run's K1 and K2 put in
               // the basis as scan_plane_class does -> disc[4] k1|K1 k2|K2 e1x e1y r²[4] (if want_r2, else 0)
        const V<R> o = v3(20), d = v3(23);
        const V<R> ud = unit(d);
        RayBasis<float, kBasisXY> b = make_basis<float, kBasisXY>(V<float>{(float)ud.x, (float)ud.y, (float)ud.z}, V<float>{(float)o.x, (float)o.y, (float)o.z});
        const float ft = (float)(R)a[26];
        const int cls = (int)a[27];
        if (cls >= 2) b.k1 = plane_run_k1((float)a[4], b.e1y, b.k1), b.k2 = plane_run_k2((float)a[4], b.e2y, b.k2);
        float out4[4];
        if (cls == 0) kat_block_discs<0>(a, b, ft, out4);
        else if (cls == 1) kat_block_discs<1>(a, b, ft, out4);
        else if (cls == 2) kat_block_discs<3>(a, b, ft, out4);
        else kat_block_discs<4>(a, b, ft, out4);
        for (int k = 0; k < 4; ++k) r[k] = (double)out4[k], r[8 + k] = a[32] != 0.0 ? (double)(float)a[28 + k] : 0.0;
        r[4] = (double)b.k1, r[5] = (double)b.k2, r[6] = (double)b.e1x, r[7] = (double)b.e1y;
        break;
    }
    case 12: { // BUCKET_DISCS_XY: BUCKET_DISCS' record through the xy basis -> disc[4] K1b K2b e1x e1y r2b[4]
        const V<R> o = v3(20), d = v3(23);
        const V<R> ud = unit(d);
        RayBasis<float, kBasisXY> b = make_basis<float, kBasisXY>(V<float>{(float)ud.x, (float)ud.y, (float)ud.z}, V<float>{(float)o.x, (float)o.y, (float)o.z});
        b.k1 = bucket_k1((float)a[27], (float)a[4], (float)(R)a[26], b.e1y, b.k1);
        b.k2 = bucket_k2((float)a[27], (float)a[4], (float)(R)a[26], b.e2y, b.k2);
        float out4[4];
        kat_block_discs<5>(a, b, 0.0f, out4);
        for (int k = 0; k < 4; ++k) r[k] = (double)out4[k], r[8 + k] = (double)(float)a[28 + k];
        r[4] = (double)b.k1, r[5] = (double)b.k2, r[6] = (double)b.e1x, r[7] = (double)b.e1y;
        break;
    }
    case 13: { // SET_DISCS: one block of a one-radius set (scan_sets): cx[8] cz[8] cy v0 . movy o(3) d(3) time (+ the set's padded
               // R2 at 36, from the host) -> disc[8] K1 K2 R2
        typedef ScanGroup<float, 6> Grp;
        const V<R> o = v3(20), d = v3(23);
        const V<R> ud = unit(d);
        RayBasis<float, kBasisXY> b = make_basis<float, kBasisXY>(V<float>{(float)ud.x, (float)ud.y, (float)ud.z}, V<float>{(float)o.x, (float)o.y, (float)o.z});
        const float v0 = (float)a[17], cy = (float)a[16], ft = (float)(R)a[26];
        if (a[19] != 0.0) b.k1 = bucket_k1(v0, cy, ft, b.e1y, b.k1), b.k2 = bucket_k2(v0, cy, ft, b.e2y, b.k2);
        else b.k1 = plane_run_k1(cy, b.e1y, b.k1), b.k2 = plane_run_k2(cy, b.e2y, b.k2);
        Grp g;
        for (int q = 0; q < Grp::H; ++q) g.cx[q] = f2{(float)a[2 * q], (float)a[2 * q + 1]}, g.cz[q] = f2{(float)a[8 + 2 * q], (float)a[9 + 2 * q]};
        float out8[Grp::G];
        g.discs(out8, b, 0.0f, (float)a[36]);
        for (int k = 0; k < Grp::G; ++k) r[k] = (double)out8[k];
        r[8] = (double)b.k1, r[9] = (double)b.k2, r[10] = (double)(float)a[36];
        break;
    }
    default: break;
    }
}

} // namespace rayz_dev
