// shade.hpp — what happens to a path at the end of a segment, and how one starts: the textures (src/material.zig:19-51), the
// background, the hit record (src/hit.zig:25-41), the scattered direction (src/material.zig:73-160,179-211), shade() that puts
// them together for the trace kernels, and the camera ray (src/camera.zig:59-90).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.hpp"
#include "device_types.hpp"

namespace rayz_dev {

// Cell parity of a checker at point p: floor(p_k / scale) summed as integers, floored mod 2 (src/material.zig:32-36;
// the reference sums i64s, here each floor is clamped to ±2^30 and summed as int32 — same parity inside that range).
template <class R> __device__ __forceinline__ uint32_t checker_parity(V<R> p, R scale) {
    const R lim = R(1073741824.0);
    R fx = fl(p.x / scale), fy = fl(p.y / scale), fz = fl(p.z / scale);
    fx = fx < -lim ? -lim : fx;
    fx = fx > lim ? lim : fx;
    fy = fy < -lim ? -lim : fy;
    fy = fy > lim ? lim : fy;
    fz = fz < -lim ? -lim : fz;
    fz = fz > lim ? lim : fz;
    const uint32_t s = (uint32_t)(int32_t)fx + (uint32_t)(int32_t)fy + (uint32_t)(int32_t)fz;
    return s & 1u;
}
template <class R, class TexPtr>
__device__ __forceinline__ V<R> texture_value(TexPtr tex, uint32_t idx, V<R> p) { // src/material.zig:19-51
    typedef typename VecOf<R>::type r4;
    for (int depth = 0; depth < kMaxTextureDepth; ++depth) { // rayz_hip_scene_create refuses deeper chains and cycles
        const r4 h = tex[2 * idx];
        if (bits(h.x) == 1u) { // RAYZ_TEX_SOLID
            const r4 c = tex[2 * idx + 1];
            return {c.x, c.y, c.z};
        }
        idx = checker_parity<R>(p, h.w) == 0u ? bits(h.y) : bits(h.z);
    }
    return {R(0), R(0), R(0)};
}

// ---- pieces of the shading step; the trace kernels use them through shade(), the known-answer entry calls them
// directly (the same instructions either way) ------------------------------------------------------------------------
// Background of a ray that hits nothing: ((1−t)·(1,1,1) + (0.5,0.7,1.0))·t, t = ½(unit(d).y + 1) — not a lerp,
// src/renderer.zig:124-125.
template <class R> __device__ __forceinline__ V<R> background(V<R> ud) {
    const R t = R(0.5) * (ud.y + R(1));
    const R w = R(1) - t;
    return {(w + R(0.5)) * t, (w + R(0.7)) * t, (w + R(1.0)) * t};
}
// Hit point, outward normal of a (moving) sphere and the front-face flip: src/geom.zig:63-65, src/hit.zig:25-41.
template <class R>
__device__ __forceinline__ void sphere_hit_record(typename VecOf<R>::type c, typename VecOf<R>::type v, V<R> o, V<R> d, R time,
                                                  R t, V<R>& pt, V<R>& nrm) {
    pt = {fm(d.x, t, o.x), fm(d.y, t, o.y), fm(d.z, t, o.z)};
    const V<R> cn{fm(v.x, time, c.x), fm(v.y, time, c.y), fm(v.z, time, c.z)};
    nrm = unit(V<R>{pt.x - cn.x, pt.y - cn.y, pt.z - cn.z});
}
template <class R> __device__ __forceinline__ bool face_forward(V<R> d, V<R>& nrm) { // Hit.init, src/hit.zig:33-36
    const bool front = dot3(nrm, d) < R(0);
    if (!front) nrm = neg(nrm);
    return front;
}
// Schlick's reflectance with pow(x, 5) as multiplies: src/material.zig:179-183.
template <class R> __device__ __forceinline__ R reflectance(R cosv, R eta) {
    R r0 = (R(1) - eta) / (R(1) + eta);
    r0 = r0 * r0;
    const R xx = R(1) - cosv;
    const R x2 = xx * xx;
    const R x5 = (x2 * x2) * xx;
    return fm(R(1) - r0, x5, r0);
}
template <class R> __device__ __forceinline__ V<R> reflect(V<R> d, V<R> nrm) { // src/material.zig:185-187
    const R k = R(2) * dot3(d, nrm);
    return {fm(-k, nrm.x, d.x), fm(-k, nrm.y, d.y), fm(-k, nrm.z, d.z)};
}
// src/material.zig:189-194 with cos = −ud·n handed in (the caller has it).  Exact arithmetic has 1 − |perp|² ≥ 0
// here (eta·sin ≤ 1); in f32 it rounds below 0 about once per 1e9 samples and the reference's bare sqrt (:192)
// would make the pixel NaN: clamped at 0.
template <class R> __device__ __forceinline__ V<R> refract(V<R> ud, V<R> nrm, R cosv, R eta) {
    const V<R> perp{fm(nrm.x, cosv, ud.x) * eta, fm(nrm.y, cosv, ud.y) * eta, fm(nrm.z, cosv, ud.z) * eta};
    const R sp = -sq(mx(R(1) - dot3(perp, perp), R(0)));
    return {fm(nrm.x, sp, perp.x), fm(nrm.y, sp, perp.y), fm(nrm.z, sp, perp.z)};
}
// `Material.scatter` (src/material.zig:73-160) without the texture lookup: the scattered direction, or false when
// a metal absorbs the ray.  `d` is the incoming direction as the ray holds it (unnormalised), `ud` = unit(d).
template <class R, class G>
__device__ __forceinline__ bool scatter_dir(uint32_t kind, uint32_t method, R param, R inv_param, G& g, V<R> d, V<R> ud, V<R> pt,
                                            V<R> nrm, bool front, V<R>& nd) {
    // Diffuse and fuzzy-metal lanes both start from a point in the unit sphere: drawn here, ONCE for the wave's lanes of
    // either kind (each lane consumes exactly the draws it would inside its own branch) — two rejection loops in two
    // divergent branches cost the wave twice its slowest lane.
    V<R> r{0, 0, 0};
    if (kind == 0u || (kind == 1u && param > R(0))) r = random_in_unit_sphere<R>(g);
    if (kind == 0u) { // diffuse, :77-101
        V<R> target;
        if (method == 2u) { // HEMISPHERE, :208-211
            if (!(dot3(r, nrm) > R(0))) r = neg(r);
            target = {pt.x + r.x, pt.y + r.y, pt.z + r.z};
        } else {
            if (method == 1u) r = unit(r); // UNIT_SPHERE_SURFACE
            target = {(pt.x + nrm.x) + r.x, (pt.y + nrm.y) + r.y, (pt.z + nrm.z) + r.z};
        }
        const R tol = (R)1e-8;
        if (ab(target.x) <= tol && ab(target.y) <= tol && ab(target.z) <= tol) target = nrm; // :85-86
        nd = {target.x - pt.x, target.y - pt.y, target.z - pt.z};
    } else if (kind == 1u) { // metallic, :108-131
        V<R> m = unit(reflect<R>(d, nrm));
        if (param > R(0)) {
            const V<R> ru = unit(r);
            const R f = param < R(1) ? param : R(1);
            m = {fm(ru.x, f, m.x), fm(ru.y, f, m.y), fm(ru.z, f, m.z)};
        }
        if (dot3(m, nrm) <= R(0)) return false; // absorbed
        nd = m;
    } else { // dielectric, :137-159
        const R eta = front ? inv_param : param;
        const R cosv = -dot3(ud, nrm);
        const R sinv = sq(fm(-cosv, cosv, R(1)));
        bool refl = eta * sinv > R(1);
        if (!refl) refl = reflectance<R>(cosv, eta) > uniform<R>(g); // the draw happens only when not TIR, :145
        nd = refl ? reflect<R>(d, nrm) : refract<R>(ud, nrm, cosv, eta);
    }
    return true;
}

// ---- shading of one segment: returns false when the path ends ------------------------------------
// On a miss adds thr ⊙ background to acc (src/renderer.zig:124-125); on absorption adds nothing.
// `ibest` is a POOL index; `ud` = unit(d) as the scan used it.
template <class R>
__device__ __forceinline__ bool shade(const DevScene<R>& sc, Pcg32& g, V<R>& o, V<R>& d, V<R> ud, R time, R tbest,
                                      int ibest, V<R>& thr, V<R>& acc) {
    typedef typename VecOf<R>::type r4;
    // The pass's three table pointers, read ONCE here: left to itself the compiler re-loads each kernel argument where it is
    // used (scalar registers are short), a scalar load + wait in front of every dependent table fetch of the pass.
    const r4* pool_gen = sc.sph_pool;
    const r4* mat_gen = sc.mat;
    const r4* tex_gen = sc.tex;
    asm volatile("" : "+s"(pool_gen), "+s"(mat_gen), "+s"(tex_gen));
    // (.. and named GLOBAL again: behind the empty asm the compiler no longer knows the address space and emits flat_load,
    //  which counts on both wait counters and resolves its aperture per lane)
    const RAYZ_GLOBAL r4* pool_p = (const RAYZ_GLOBAL r4*)pool_gen;
    const RAYZ_GLOBAL r4* mat_p = (const RAYZ_GLOBAL r4*)mat_gen;
    const RAYZ_GLOBAL r4* tex_p = (const RAYZ_GLOBAL r4*)tex_gen;
    if (ibest < 0) {
        const V<R> col = background<R>(ud);
        acc.x = acc.x + thr.x * col.x;
        acc.y = acc.y + thr.y * col.y;
        acc.z = acc.z + thr.z * col.z;
        return false;
    }
    // hit record: src/geom.zig:63-65, src/hit.zig:25-41 (spheres); geometric normal for triangles
    V<R> pt, nrm;
    uint32_t mat_idx;
    if ((uint32_t)ibest < sc.n_spheres) {
        const r4 q = pool_p[2 * ibest], w4 = pool_p[2 * ibest + 1];
        sphere_hit_record<R>(q, w4, o, d, time, tbest, pt, nrm);
        mat_idx = bits(w4.w);
    } else {
        const uint32_t ti = (uint32_t)ibest - sc.n_spheres;
        const r4 a = sc.tri[3 * ti], b = sc.tri[3 * ti + 1], c = sc.tri[3 * ti + 2];
        pt = {fm(d.x, tbest, o.x), fm(d.y, tbest, o.y), fm(d.z, tbest, o.z)};
        nrm = unit(cross3(V<R>{b.x, b.y, b.z}, V<R>{c.x, c.y, c.z}));
        mat_idx = bits(a.w);
    }
    const bool front = face_forward<R>(d, nrm);

    const r4 m = mat_p[mat_idx];
    const uint32_t kind = bits(m.x) & 0xffu, method = (bits(m.x) >> 8) & 0xffu, texture = bits(m.y);
    V<R> nd;
    if (!scatter_dir<R>(kind, method, m.z, m.w, g, d, ud, pt, nrm, front, nd)) return false;
    const V<R> att = kind == 2u ? V<R>{R(1), R(1), R(1)} : texture_value<R>(tex_p, texture, pt);
    thr = {thr.x * att.x, thr.y * att.y, thr.z * att.z};
    o = pt;
    d = nd;
    return true;
}

// ---- camera ray of path (px, py, s): src/camera.zig:59-90 ---------------------------------------
template <class R, class G>
__device__ __forceinline__ void camera_ray(const DevCamera<R>& cam, G& g, uint32_t px, uint32_t py, V<R>& o, V<R>& d,
                                           R& time) {
    const R x = (R)px + (uniform<R>(g) - R(0.5));
    const R y = (R)py + (uniform<R>(g) - R(0.5));
    o = {cam.from[0], cam.from[1], cam.from[2]};
    if (cam.defocus) {
        R vx = 0, vy = 0;
        for (int i = 0; i < kMaxRejectionTries; ++i) {
            vx = fm(uniform<R>(g), R(2), R(-1));
            vy = fm(uniform<R>(g), R(2), R(-1));
            if (fm(vy, vy, vx * vx) <= R(1)) break;
        }
        o.x = cam.from[0] + fm(cam.defv[0], vy, cam.defu[0] * vx);
        o.y = cam.from[1] + fm(cam.defv[1], vy, cam.defu[1] * vx);
        o.z = cam.from[2] + fm(cam.defv[2], vy, cam.defu[2] * vx);
    }
    d.x = (fm(cam.dv[0], y, cam.du[0] * x) + cam.pxo[0]) - o.x;
    d.y = (fm(cam.dv[1], y, cam.du[1] * x) + cam.pxo[1]) - o.y;
    d.z = (fm(cam.dv[2], y, cam.du[2] * x) + cam.pxo[2]) - o.z;
    time = uniform<R>(g);
}

// `getRay(px, py, null)` (src/camera.zig:59-77 with rng == null: the pixel's centre, the lens centre, time 0) — the form the
// reference's own "get ray" test calls (src/renderer.zig:129-149).  No path ever takes it (the kernels always draw); it exists for
// the known-answer entry, in the same operation order as camera_ray above.
template <class R> __device__ __forceinline__ void camera_ray_no_rng(const DevCamera<R>& cam, uint32_t px, uint32_t py, V<R>& o, V<R>& d, R& time) {
    const R x = (R)px, y = (R)py;
    o = {cam.from[0], cam.from[1], cam.from[2]};
    d.x = (fm(cam.dv[0], y, cam.du[0] * x) + cam.pxo[0]) - o.x;
    d.y = (fm(cam.dv[1], y, cam.du[1] * x) + cam.pxo[1]) - o.y;
    d.z = (fm(cam.dv[2], y, cam.du[2] * x) + cam.pxo[2]) - o.z;
    time = R(0);
}

} // namespace rayz_dev
