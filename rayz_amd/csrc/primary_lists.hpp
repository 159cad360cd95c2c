// primary_lists.hpp — which spheres a pixel's camera rays can hit at all.  Every path of a pixel starts
// with a ray from the lens through the pixel's square of the focus plane at a time in [0, 1): the spheres such a ray can meet
// are a fact of (scene, camera, pixel), not of the sample.  may_hit() is the conservative test primary_lists_kernel
// (trace_kernels_flat.hpp) builds each pixel's list with; the trace kernels compiled with RAYZ_TRACE_KERNEL_PRIMARY resolve a path's
// camera segment from the list (narrow_eval decides, as it does behind the scan) instead of scanning the whole flat list.
// The test only has to be a SUPERSET: it is f64 throughout, host and device, and every inequality carries its margin.
// Also compiled by the host compiler alone (tests/primary_lists_mirror.cpp).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RAYZ_PL_HD __host__ __device__ __forceinline__
#else
#define RAYZ_PL_HD inline
#endif

namespace rayz_primary {

// A pixel's record holds its count and up to kListK slot numbers; a pixel with more candidates has kNoList as its count and takes
// its camera segment through the scan.  Records are stored by field: word j of local pixel i at [j · pixels + i], j = 0 the count.
// kListK: the smallest of {8, 16, 32} that leaves at most 5 % of the headline frame's pixels without a list
// (profiles/r15/primary_lists/README.md has the histogram).
constexpr uint32_t kListK = 32;
constexpr uint32_t kNoList = 0xffffffffu;

// AUTO's two gates, kPrimaryMinSpheres and kPrimaryMinSpp, stand beside kSetPayoffSlots in plane_runs.hpp with the figures they
// were read from.

// The camera as camera_ray (shade.hpp) reads it, in f64.
struct BeamCamera {
    double from[3], du[3], dv[3], pxo[3], defu[3], defv[3];
    uint32_t defocus;
};

// Margins.  kRel: the f64 roundings of this file's own arithmetic (each a few 2^-53 relative).  kF32: what the f32 kernels add
// — DevCamera<float> holds the camera narrowed to f32 and camera_ray forms o and d in f32, each rounding at most 2^-24 of the
// magnitudes involved; 2^-20 of their sum covers sixteen of them.  kJitter: the f32 pixel coordinate px + (u − ½) is rounded
// at px's magnitude: by at most 2^-8 of a pixel in a frame of up to 65,536 pixels a side, which is 2^-7 of the pixel
// square's half width.
constexpr double kRel = 1e-9, kF32 = 0x1p-20, kJitter = 0x1p-7;

RAYZ_PL_HD double norm3(const double* v) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// What may_hit needs of a pixel: the axis (from the lens centre O through the pixel centre P: O + l·u, l the arc length, |P − O| = L)
// and the bounds A ≥ |a|, B ≥ |b| of the derivation (§4.19), margins included.  wide: the beam is no narrow one (the lens and
// the pixel square are not small against the focus distance, the camera is not finite, or the pixel lies beyond the 65,536 columns
// and rows kJitter is good for): every sphere is kept.
struct PixelBeam {
    double o[3], u[3], L, A, B;
    bool wide;
};

RAYZ_PL_HD PixelBeam pixel_beam(const BeamCamera& c, uint32_t px, uint32_t py) {
    PixelBeam b;
    double d[3];
    for (int k = 0; k < 3; ++k) {
        b.o[k] = c.from[k];
        d[k] = (c.pxo[k] + c.du[k] * (double)px + c.dv[k] * (double)py) - c.from[k];
    }
    b.L = norm3(d);
    const double lens = c.defocus ? norm3(c.defu) + norm3(c.defv) : 0.0;
    const double nu = norm3(c.du), nv = norm3(c.dv);
    // the magnitudes the f32 forms of o and of the focus-plane point are rounded at
    const double M = norm3(c.from) + norm3(c.pxo) + nu * ((double)px + 1.0) + nv * ((double)py + 1.0) + lens;
    b.A = lens * (1.0 + kRel) + kF32 * M;
    b.B = 0.5 * (nu + nv) * (1.0 + kJitter) + kF32 * M;
    b.wide = !(b.L > 2.0 * (b.A + b.B)) || !(b.L < 1e300) || px >= 65536u || py >= 65536u; // (kJitter's frame bound)
    const double inv = b.wide ? 0.0 : 1.0 / b.L;
    for (int k = 0; k < 3; ++k) b.u[k] = d[k] * inv;
    return b;
}

// Squared distance from q (relative to the axis origin) to the axis points of arc length l0 .. l1.  Whatever l the clamp
// gives, the result is the squared distance to SOME point of that stretch evaluated in f64: never below the true minimum by
// more than its own rounding (the callers' slack2).
RAYZ_PL_HD double axis_dist2(const double* q, const double* u, double l0, double l1) {
    double l = q[0] * u[0] + q[1] * u[1] + q[2] * u[2];
    l = l < l0 ? l0 : l;
    l = l > l1 ? l1 : l;
    const double ex = q[0] - l * u[0], ey = q[1] - l * u[1], ez = q[2] - l * u[2];
    return ex * ex + ey * ey + ez * ez;
}

// Pieces the sweep c + v·t, t in [0, 1], of a moving sphere is cut into: each piece lies in the ball of radius |r| + |v| / (2 n)
// about its middle.
constexpr int kSweepPieces = 8;

// True whenever some camera ray of the beam's pixel — any lens point of the square, any point of the pixel square, any time
// in [0, 1] — meets the sphere (centre c, velocity v, radius r of either sign) at some t > 0.  The proof is DESIGN.md §4.19.
RAYZ_PL_HD bool beam_may_hit(const PixelBeam& b, const double* c, const double* v, double r) {
    if (b.wide) return true;
    const double ra = fabs(r), vn = norm3(v);
    double qm[3], q0[3];
    for (int k = 0; k < 3; ++k) {
        q0[k] = c[k] - b.o[k];
        qm[k] = q0[k] + 0.5 * v[k];
    }
    const double rho = ra + 0.5 * vn, D = norm3(qm);
    // arc length no hit lies beyond: a hit point is within D + rho of the lens centre and, at s ≥ 1, at least s·(L − A − B) from it
    double lmax = (D + rho) * (b.L / (b.L - b.A - b.B)) * (1.0 + kRel);
    lmax = lmax > b.L ? lmax : b.L;
    const double S = lmax / b.L * (1.0 + kRel);
    // half widths of the beam: A(1 − s) + B s on s in [0, 1], A(s − 1) + B s on [1, S]
    const double W1 = b.A > b.B ? b.A : b.B;
    const double wS = b.A * (S - 1.0) + b.B * S;
    const double W2 = b.B > wS ? b.B : wS;
    const double Wm = W1 > W2 ? W1 : W2;
    // rounding of the squared distances here and of narrow_eval's discriminant: far below 1e-12 of the squared lengths involved
    const double Q = D + rho + b.A + lmax;
    const double slack2 = 1e-12 * Q * Q;
    const double Rm = (rho + Wm) * (1.0 + kRel);
    if (axis_dist2(qm, b.u, 0.0, lmax) > Rm * Rm + slack2) return false; // the ball of the whole sweep is out of reach
    const int n = vn == 0.0 ? 1 : kSweepPieces;
    const double h = vn / (2.0 * n);
    const double R1 = (ra + h + W1) * (1.0 + kRel), R2 = (ra + h + W2) * (1.0 + kRel);
    for (int i = 0; i < n; ++i) {
        const double t = ((double)i + 0.5) / (double)n;
        const double q[3] = {q0[0] + v[0] * t, q0[1] + v[1] * t, q0[2] + v[2] * t};
        if (!(axis_dist2(q, b.u, 0.0, b.L) > R1 * R1 + slack2)) return true;
        if (!(axis_dist2(q, b.u, b.L, lmax) > R2 * R2 + slack2)) return true;
    }
    return false;
}

RAYZ_PL_HD bool may_hit(const BeamCamera& cam, uint32_t px, uint32_t py, const double* c, const double* v, double r) {
    return beam_may_hit(pixel_beam(cam, px, py), c, v, r);
}

} // namespace rayz_primary
