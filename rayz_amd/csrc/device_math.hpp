// device_math.hpp — the arithmetic every device function is written with: the one-rounding helpers (fm, mx, mn, sq, fl, ab, bits),
// the acceptance rule of every narrow phase (accept_root), a u32 carried in an R (Bits), the vector V with dot3 / unit / cross3, and
// both random generators (Pcg32, one stream per path; ListRng, the known-answer entry's) with uniform and
// random_in_unit_sphere.  "Mode B" of DESIGN.md §4: FMAs appear only where written.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_types.hpp"

namespace rayz_dev {

// ---- small helpers -----------------------------------------------------------------------------
__device__ __forceinline__ float fm(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fm(double a, double b, double c) { return __builtin_fma(a, b, c); }
__device__ __forceinline__ float mx(float a, float b) { return __builtin_fmaxf(a, b); }
__device__ __forceinline__ double mx(double a, double b) { return __builtin_fmax(a, b); }
__device__ __forceinline__ float sq(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ double sq(double x) { return __builtin_sqrt(x); }
__device__ __forceinline__ float fl(float x) { return __builtin_floorf(x); }
__device__ __forceinline__ double fl(double x) { return __builtin_floor(x); }
__device__ __forceinline__ float ab(float x) { return __builtin_fabsf(x); }
__device__ __forceinline__ double ab(double x) { return __builtin_fabs(x); }
__device__ __forceinline__ uint32_t bits(float x) { return __builtin_bit_cast(uint32_t, x); }
__device__ __forceinline__ uint32_t bits(double x) { return (uint32_t)__builtin_bit_cast(uint64_t, x); }

// The acceptance rule of every narrow phase: a root in range that is nearer, or as near with the larger hittable
// index.  Written with & and | on purpose: `&&` / `||` make the compiler branch per term (five s_and_saveexec / s_cbranch_execz
// pairs around two moves in the candidates' phase); this is four compares, three scalar mask operations and two selects.
#ifndef RAYZ_BRANCHY_ACCEPT
template <class R> __device__ __forceinline__ void accept_root(R t, int index, R tmin, R& tbest, int& ibest) {
    const bool take = (t >= tmin) & ((t < tbest) | ((t == tbest) & (index > ibest)));
    tbest = take ? t : tbest;
    ibest = take ? index : ibest;
}
#else
template <class R> __device__ __forceinline__ void accept_root(R t, int index, R tmin, R& tbest, int& ibest) {
    if (t >= tmin && (t < tbest || (t == tbest && index > ibest))) {
        tbest = t;
        ibest = index;
    }
}
#endif

template <class R> struct Bits; // a u32 carried in the bits of an R
template <> struct Bits<float> {
    static __host__ __device__ __forceinline__ float from(uint32_t u) { return __builtin_bit_cast(float, u); }
};
template <> struct Bits<double> {
    static __host__ __device__ __forceinline__ double from(uint32_t u) { return __builtin_bit_cast(double, (uint64_t)u); }
};

template <class R> struct V {
    R x, y, z;
};
template <class R> __device__ __forceinline__ R dot3(V<R> a, V<R> b) { return fm(a.z, b.z, fm(a.y, b.y, a.x * b.x)); }
template <class R> __device__ __forceinline__ V<R> neg(V<R> a) { return {-a.x, -a.y, -a.z}; }
template <class R> __device__ __forceinline__ V<R> unit(V<R> a) {
    const R m = sq(dot3(a, a));
    const R inv = R(1) / m;
    return {a.x * inv, a.y * inv, a.z * inv};
}

// ---- PCG32 (XSH-RR 64/32), one stream per path: DESIGN.md §4.1 ---------------------------------
__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}
struct Pcg32 {
    unsigned long long state, inc;
    __device__ __forceinline__ uint32_t next() {
        const unsigned long long old = state;
        state = old * 6364136223846793005ull + inc;
        const uint32_t xorshifted = (uint32_t)(((old >> 18u) ^ old) >> 27u);
        const uint32_t rot = (uint32_t)(old >> 59u);
        return (xorshifted >> rot) | (xorshifted << ((32u - rot) & 31u));
    }
    __device__ __forceinline__ void seed_path(unsigned long long seed, unsigned long long path_id) {
        const unsigned long long a = mix64(seed + (path_id + 1) * 0x9e3779b97f4a7c15ull);
        const unsigned long long b = mix64(a + 0x9e3779b97f4a7c15ull);
        state = 0;
        inc = (b << 1) | 1u;
        next();
        state += a;
        next();
    }
};
template <class R> __device__ __forceinline__ R uniform(Pcg32& g);
template <> __device__ __forceinline__ float uniform<float>(Pcg32& g) { return (float)(g.next() >> 8) * 0x1p-24f; }
template <> __device__ __forceinline__ double uniform<double>(Pcg32& g) { return (double)g.next() * 0x1p-32; }
// Known-answer entry (rayz_hip_kat) only: draws come from a caller-supplied list, so that the device functions can
// be evaluated on the same uniforms as the reference restatement (0.5 once the list is used up).
struct ListRng {
    const double* u;
    uint32_t n, i;
};
template <class R> __device__ __forceinline__ R uniform(ListRng& g) {
    const R v = g.i < g.n ? (R)g.u[g.i] : R(0.5);
    g.i++;
    return v;
}

template <class R, class G> __device__ __forceinline__ V<R> random_in_unit_sphere(G& g) { // src/material.zig:196-202
    V<R> v{0, 0, 0};
    for (int i = 0; i < kMaxRejectionTries; ++i) {
        v.x = fm(uniform<R>(g), R(2), R(-1));
        v.y = fm(uniform<R>(g), R(2), R(-1));
        v.z = fm(uniform<R>(g), R(2), R(-1));
        // `v.mag() <= 1` (src/material.zig:199) without the square root: for a correctly rounded sqrt,
        // sqrt(x) <= 1  <=>  x <= nextafter(1): sqrt(1 + ulp) = 1 + ulp/2 - ulp²/8 lies below the midpoint and rounds to 1,
        // sqrt(1 + 2 ulp) rounds to 1 + ulp.  Same decision, bit for bit, as the oracle's literal form.
        if (dot3(v, v) <= (sizeof(R) == 4 ? R(0x1.000002p0f) : R(0x1.0000000000001p0))) break;
    }
    return v;
}

template <class R, int N> __device__ __forceinline__ R max_of(const R (&v)[N]) {
    R m = v[0];
#pragma unroll
    for (int k = 1; k < N; ++k) m = mx(m, v[k]);
    return m;
}

template <class R> __device__ __forceinline__ V<R> cross3(V<R> a, V<R> b) {
    return {fm(a.y, b.z, -(a.z * b.y)), fm(a.z, b.x, -(a.x * b.z)), fm(a.x, b.y, -(a.y * b.x))};
}
__device__ __forceinline__ float mn(float a, float b) { return __builtin_fminf(a, b); }
__device__ __forceinline__ double mn(double a, double b) { return __builtin_fmin(a, b); }

} // namespace rayz_dev
