// rayz_device.hpp — gfx950 device code of the render path (included by rayz_hip.hip only).
//
// One work-item per pixel-sample path.  A wave keeps 64 paths in flight and re-fills finished lanes
// from a global work queue (wave64 ballot + mbcnt prefix ranks, one atomic per wave), so the sphere
// scan — ≥95 % of the time on a flat hit list — always runs with a full EXEC mask.  The scan is
// wave-uniform over the sphere index: sphere records come through the SCALAR path (s_load_dwordx4/x8
// from a constant-address-space pointer) and feed the VALU as SGPR operands, which costs no VGPRs, no
// LDS bandwidth and no 64× replicated vector loads.  Arithmetic is the "mode B" specification of
// DESIGN.md §4; every statement below has its twin in oracle/rayz_oracle.cpp namespace B, and the two
// must agree bit for bit (build with -ffp-contract=off: FMAs appear only where written).
//
// Reference semantics restated here (file:line into jlucier/rayz):
//   camera ray      src/camera.zig:59-90      sphere test   src/geom.zig:38-66
//   hit record      src/hit.zig:25-41         scatter       src/material.zig:73-160,179-211
//   textures        src/material.zig:19-51    bounce loop   src/renderer.zig:103-126 (recursion → loop)
//   pixel mean      src/renderer.zig:86-95
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plane_runs.hpp"
#include "primary_lists.hpp"
#include "slab_cells.hpp"

namespace rayz_dev {

#define RAYZ_CONSTANT __attribute__((address_space(4)))
#define RAYZ_GLOBAL __attribute__((address_space(1)))

typedef float f4 __attribute__((ext_vector_type(4)));
typedef double d4 __attribute__((ext_vector_type(4)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef float f2 __attribute__((ext_vector_type(2)));
typedef double d2 __attribute__((ext_vector_type(2)));

constexpr int kMaxRejectionTries = 64;
constexpr int kMaxTextureDepth = 8;
#ifndef RAYZ_GROUP
#define RAYZ_GROUP 4
#endif
// spheres per scan group (and per SoA block of a stream): 4 — the two ping-pong SGPR sets of a y-moving group are
// 2 x 5 x G registers, and more than ~40 SGPRs spill inside the loop.  (The scan streams are f32 for both precisions;
// group_size<double> = 2 belonged to the f64 streams the f64 kernel scanned until round 2.)
template <class R> constexpr int group_size() { return sizeof(R) == 8 ? RAYZ_GROUP / 2 : RAYZ_GROUP; }
constexpr int kStaticGroup = RAYZ_GROUP; // A stream is padded to a whole
constexpr int kMovYGroup = RAYZ_GROUP;   //   number of group PAIRS plus two spare groups, so that the prefetch of the
constexpr int kMovGGroup = 2;   //   next group never leaves the array.
constexpr int kTriGroup = 2;

template <class R> struct VecOf;
template <> struct VecOf<float> { typedef f4 type; typedef f2 pair; };
template <> struct VecOf<double> { typedef d4 type; typedef d2 pair; };

// ---- device-resident scene (HBM layout) ------------------------------------------
// Scan streams, one per velocity class, each padded with never-hit records (r² = -inf):
//   static  v = 0            stat: blocks of G = 4 spheres, SoA inside a block:
//                                  cx[G] cy[G] cz[G] r²[G]
//   mov-Y   v = (0, vy, 0)   movy: blocks of G: cx[G] cy[G] cz[G] r²[G] vy[G]
//                            (what randomBouncing makes)
//   mov-G   any other v      movg[2i] = {cx, cy, cz, r²}, movg[2i+1] = {vx, vy, vz, 0}
// Inside the static and mov-Y classes, spheres that share one f32 centre height cy (randomBouncing puts its whole grid at
// y = 0.2) are gathered into PLANE RUNS, which come first in the class's stream and slot order: blocks of G without the
// cy field, cx[G] cz[G] r²[G] (+ vy[G]); the run's cy is held once, in the stream's head.  Per stream:
//   [head][plane blocks of run 0, run 1, ...][two spare plane groups][loose blocks, the layout above][two spare groups]
// The stream's head (kPlaneHeader words) holds its layout: {number of runs, plane_slots = the slots the runs cover, 0, 0},
// then kMaxPlaneRuns PlaneRun records (mov-Y: words 2, 3 = the bucket section, below).  It is read with scalar loads at every scan: a run table in the kernel arguments
// indexed by the run counter is copied to scratch, and any new argument is loaded once per kernel and held (spilled)
// across the whole persistent loop.
// The block layout puts the same field of two neighbouring spheres in one aligned SGPR pair, which is what a
// v_pk_fma_f32 takes as a single scalar operand.  A "slot" numbers the records stat | movy | movg
// in that order.  All three are f32 for both precisions (the reject test only filters); the f64
// copies feed the narrow phase.
using rayz_plane::kMaxPlaneRuns;
using rayz_plane::PlaneRun;
constexpr int kPlaneHeader = 16; // words of layout at the head of the static and mov-Y streams (64 B: blocks stay aligned)
static_assert(4 * sizeof(uint32_t) + kMaxPlaneRuns * sizeof(PlaneRun) <= kPlaneHeader * sizeof(float), "run table fits the head");
// SPEED BUCKETS (mov-Y stream only; rayz_plane::plan_buckets): the members of a y-moving run whose f32 vy lie
// within r_min / 8 of each other are tested with ONE speed v0, folded into the ray's K2 as the run's height is, against a radius
// grown by |vy − v0|: the static plane form, 6 packed FMAs per sphere pair.  A run's slots are its buckets' (by speed), then
// the members no bucket took, in the run's own 4-field blocks, then its pads.  Behind the loose section the stream carries
//   [kBucketHeader words: per run, the first slot of its 4-field remainder][SpeedBucket records][the buckets' blocks
//    cx[G] cz[G] r2b[G], back to back][two spare groups]
// and the head's words 2 and 3 hold that section's word offset and the number of buckets.  Read with scalar loads at every
// scan, as the run table is and for its reasons.
// ONE-RADIUS SETS (both streams; rayz_plane::plan_sets): the members of a static run, or of one speed bucket, whose
// |radius| + h lie within r_min / 16 of each other are tested with ONE padded r², the set's.  A run's or bucket's slots are its
// sets' (by radius), then the members no set took, in the blocks they always had (a set's slots keep their blocks there too: the
// XZ and XY kernels, adaptive passes and queries scan those).  Behind everything above, at the next 64-byte boundary, the stream
// carries the set section, which only flat_one_radius_kernel reads:
//   [kSetHeader words: sets, bucket records, 0, 0, per run the first slot its old form still tests][RadiusSet records]
//   [the SpeedBucket records once more, `first` = the first slot the bucket's old form still tests][to a 64-byte boundary]
//   [the sets' blocks cx[8] cz[8], back to back][two spare groups]
// Nothing in front of it moves or changes; the kernel finds it from the stream's length, which the head (and the last bucket record)
// already give (scan_plane_class).
using rayz_plane::SpeedBucket;
constexpr int kBucketHeader = 8;
static_assert(sizeof(SpeedBucket) == 32 && kMaxPlaneRuns <= kBucketHeader, "bucket table layout");

template <class R> struct DevScene {
    typedef typename VecOf<R>::type r4;
    const float* stat;       // head, plane runs, loose spheres (above)   (the scan streams are f32 for both precisions: the reject test
                             //                               only filters, the narrow phase decides — DESIGN.md §4.3)
    const float* movy;       // head, plane runs, loose spheres
    const f4* movg;
    const d4* slot64;        // [2 * slots] the pool's own f64 values per slot: {cx, cy, cz, r²}, {vx, vy, vz, 0}
    const uint32_t* slot_pool; // [slots] pool index of each slot
    const r4* sph_pool;      // [2 * n_spheres] by POOL index: {cx, cy, cz, r²}, {vx, vy, vz, bits(material)}
    const r4* mat;           // [n_mat] {bits(kind | method << 8), bits(texture), param, 1/param}
    const r4* tex;           // [2 * n_tex] {bits(kind), bits(even), bits(odd), scale}, {r, g, b, 0}
    uint32_t ns_pad, ny_pad, ng_pad, n_spheres; // slots of each class (plane runs and loose spheres together)
    // build-defined triangles (hittable index = n_spheres + i): {v0, bits(material)}, {e1 = v1 - v0, 0}, {e2 = v2 - v0, 0};
    // pool order, padded with degenerate records (e1 = e2 = 0: det = 0, never accepted) like the sphere streams
    const r4* tri;           // [3 * (nt_pad + kTriGroup)]
    uint32_t nt_pad, n_triangles;
    // BVH traversal (RAYZ_TRAVERSAL_BVH): the reference's tree in depth-first pre-order, DESIGN.md §6
    const f4* bvh_nodes;     // per INNER node, its two children's boxes for BOTH precisions (the box test only culls, §4.8), in one
                             // of two formats (bvh_quantized; the host picks by tree size, rayz_hip.hip: use_quantized_nodes):
                             //  * f32 planes, 64 B = four 16-B loads:
                             //      {L.lo.xyz, bits(L.ref)}, {L.hi.xyz, 0}, {R.lo.xyz, bits(R.ref)}, {R.hi.xyz, 0}
                             //  * 16-bit plane indices on a scene-wide grid (plane = bvh_glo[k] + index · bvh_cell[k]; lower
                             //    planes rounded down, upper ones up), 32 B = two loads:
                             //      {L.lo.x | L.hi.x << 16, L.lo.y | L.hi.y << 16, L.lo.z | L.hi.z << 16, bits(L.ref)}, {R ...}
                             //    Half the bytes: the walk is bound by the vector-memory address pipe, which works per
                             //    instruction and per byte requested (profiles/r03/lds_top), and twice as many records fit
                             //    the LDS top — at the price of 12 conversions per step: it pays for trees much larger than
                             //    the LDS top (config 5: +7.7 %), not for those the top mostly covers (config 3: −2.7 %)
                             //   ref = the child's record's byte offset (index << 6 or << 5), or
                             //         kBvhLeafFlag | first << 4 | type1 << 3 | type0 << 2 | count
    float bvh_glo[3], bvh_cell[3]; // the grid of the plane indices (f32 planes: glo = 0, cell = 1 — a plane IS its "index")
    const r4* bvh_leaf;      // [stride * slots] leaf order.  sphere: {c, r²}, {v, bits(hittable)};
                             //                  triangle: {v0, bits(hittable)}, {e1, 0}, {e2, 0}
    const d4* bvh_sph64;     // [2 * slots] leaf order, sphere slots only: {c, r²}, {v, 0}
    uint32_t bvh_n_nodes, bvh_leaf_stride; // bvh_n_nodes = number of inner-node records (0: nothing in the tree)
    // oversized hittables kept out of the tree (bvh_build.hpp), tested once per segment before the walk: up to 4 leaf
    // descriptors (first << 4 | type1 << 3 | type0 << 2 | count) naming slots after the tree's own in bvh_leaf / bvh_sph64
    uint32_t bvh_n_big_leaves, bvh_big[4];
    // the first bvh_top / 64 inner-node records (the top levels of the tree, numbered breadth-first) are copied to LDS by
    // every workgroup: a quarter of all box steps then read their node in ~100 cycles instead of a global round trip.
    // In BYTES, as inner references are (index << 6).
    uint32_t bvh_top;
};

template <class R> struct DevCamera {
    R from[3], du[3], dv[3], pxo[3], defu[3], defv[3];
    uint32_t defocus, _pad;
};

template <class R> struct TraceArgs {
    DevScene<R> sc;
    DevCamera<R> cam;
    typename VecOf<R>::type* partial; // [total_items] chunk sums
    unsigned long long* counters;     // [0] work-queue head, [1] segments, [2] node tests, [3] sphere tests (BVH)
    unsigned long long seed;
    R tmin;
    uint32_t width, height, spp, max_bounces;
    const uint32_t* chunk_start; // [chunks_per_px + 1] first sample of every chunk of a pixel (the chunk schedule)
    uint32_t chunks_per_px;
    uint32_t chunk_uniform, chunk_n_uniform; // the table's uniform prefix: chunk k < chunk_n_uniform covers samples k·chunk_uniform .. (k+1)·chunk_uniform
    uint32_t tile_rows, shard_index, shard_count, shard_pixels;
    uint32_t tiled_pixels;   // the first this-many local pixels are dealt to the queue as 8x8 tiles (place_item)
    uint32_t total_items;
    uint32_t bvh_keep;       // BVH kernel: keep_active | keep_stepping << 8 (see trace_kernel_bvh)
    uint32_t bvh_top_words;   // BVH kernel: u32s of LDS taken by the copy of the tree's top (the per-lane stacks follow)
    uint32_t bvh_big_words;   // BVH kernel: where (in u32s of LDS) the oversized hittables' records are kept, after the stacks
    uint32_t queue_grab;     // work items a wave reserves per atomic on the queue head (kQueueGrab; scheduling only)
    // adaptive passes only (read by the kAdaptive instantiations alone): the row-major local pixels still traced.
    // Entry e = k · n_active + j covers chunk k of pixel active_list[j], and its sum is stored at e: total_items = n_active · chunks
    uint32_t n_active;
    const uint32_t* active_list;
#ifdef RAYZ_EXPERIMENTS // (kept out of the product kernels' argument block: every field costs scalar registers in all of them)
    uint32_t x_words;        // exchange kernel (trace_kernel_bvhx): where (in u32s of LDS) its exchange area starts
    uint32_t x_slots;        //   ray slots per walker wave
    uint32_t x_cfg;          //   scheduling: exchange when this many lanes finished | shader's minimum batch << 8 | its patience << 16 | priorities << 24
#endif
};

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

// ---- per-path state of one of a lane's rays, and the steps every trace kernel shares ---------------------
template <class R> struct PathState {
    Pcg32 g;
    V<R> o, d, thr, acc;
    R time;
    uint32_t item, px, py, s_cur, s_end, seg;
    bool has_item, alive;
};
template <class R> __device__ __forceinline__ void path_init(PathState<R>& p) {
    p.g = Pcg32{0, 1};
    p.o = {R(0), R(0), R(0)};
    p.d = {R(0), R(0), R(1)};
    p.thr = {R(1), R(1), R(1)};
    p.acc = {R(0), R(0), R(0)};
    p.time = R(0);
    p.item = p.px = p.py = p.s_cur = p.s_end = p.seg = 0;
    p.has_item = p.alive = false;
}
// Samples of chunk k (the chunk schedule).  Every schedule starts with a run of equal chunks — all of it for a
// uniform one, all but the halving tail for the automatic one — and the host hands over that run's size and length: a lane
// that pops an item of the run computes its bounds; only the tail's few items read the table (two dependent loads in the
// refill of a pass whenever some lane pops — with 32-sample chunks that is every second pass).
template <class R> __device__ __forceinline__ void chunk_bounds(const TraceArgs<R>& A, uint32_t k, uint32_t& s0, uint32_t& s1) {
    if (k < A.chunk_n_uniform) {
        s0 = k * A.chunk_uniform;
        s1 = s0 + A.chunk_uniform;
    } else {
        s0 = A.chunk_start[k];
        s1 = A.chunk_start[k + 1];
    }
}

// ---- the work queue, as a wave sees it ------------------------------------------------------------------------
// Items come off one global counter.  A wave does not pay an atomic per refill (one word takes ≈88 atomics per µs on this
// chip: with the short items of a small scene the queue head, not the tracing, set the pace — 100 spheres ran at 3.8
// instead of 5.7 Gsamples/s at 64 spp): it reserves kQueueGrab consecutive items at a time and hands them to its lanes
// as they fall idle (ballot → prefix rank), touching the counter again only when the reserve runs out.  All fields are
// wave-uniform.  Which lane traces an item never affects the image.
// Which pixel and chunk a queue entry is: entry e = k · shard_pixels + i covers chunk k of the i-th pixel dealt.  Pixels are
// dealt in 8x8 TILES of the shard's local rows (the first A.tiled_pixels of them: whole tiles only, the rest row by row), so
// that the 64 items a wave grabs together are neighbours in both directions: their primary rays walk the same part of the
// tree (+1 … 2.6 % through the BVH, profiles/r03/tree/tile8.log).  The sums are stored by ROW-MAJOR pixel as before: `item`
// becomes k · shard_pixels + (local row · width + column), what resolve_kernel reads.  Returns k.
// (kTiled = false — the flat-list kernel, whose lanes all scan the same list: rows as they come.)
// kAdaptive (an adaptive pass, §4.14): entry e = k · n_active + j is chunk k of the j-th ACTIVE pixel; the list holds row-major
// local pixels in dealing order already, and `item` stays the compact index e.  The caller's queue guard (queue_pop: mine <
// total_items = n_active · chunks) is what keeps j inside the list.
template <class R, bool kTiled, bool kAdaptive = false>
__device__ __forceinline__ uint32_t place_item(const TraceArgs<R>& A, uint32_t& item, uint32_t& px, uint32_t& py) {
    const uint32_t per_chunk = kAdaptive ? A.n_active : A.shard_pixels;
    const uint32_t k = item / per_chunk;
    uint32_t lp = item - k * per_chunk;
    if (kAdaptive) {
        lp = A.active_list[lp];
    } else if (kTiled && lp < A.tiled_pixels) {
        const uint32_t tile = lp >> 6, w8 = A.width >> 3, trow = tile / w8, tcol = tile - trow * w8;
        lp = (trow * 8u + ((lp >> 3) & 7u)) * A.width + tcol * 8u + (lp & 7u);
        item = k * A.shard_pixels + lp;
    }
    const uint32_t lr = lp / A.width;
    px = lp - lr * A.width;
    const uint32_t tl = lr / A.tile_rows, within = lr - tl * A.tile_rows;
    py = (tl * A.shard_count + A.shard_index) * A.tile_rows + within;
    return k;
}

struct WaveQueue {
    uint32_t base = 0, count = 0; // the wave's reserve: items base .. base+count-1
    bool drained = false;         // the last reservation reached the end of the queue
};
constexpr uint32_t kQueueGrab = 64;
template <class R> __device__ __forceinline__ bool queue_empty(const WaveQueue& wq, const TraceArgs<R>& A) {
    return wq.drained && (wq.count == 0u || wq.base >= A.total_items);
}
// Every lane calls this; lanes with `need` get the next items (true + `item`) while the queue lasts.
template <class R>
__device__ __forceinline__ bool queue_pop(const TraceArgs<R>& A, WaveQueue& wq, uint32_t lane, bool need, uint32_t& item) {
    const unsigned long long need_mask = __ballot(need);
    if (need_mask == 0ull) return false;
    const uint32_t n_need = (uint32_t)__popcll(need_mask);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need_mask, 0u));
    unsigned long long mine;
    if (wq.count >= n_need) {
        mine = (unsigned long long)wq.base + rank;
        wq.base += n_need;
        wq.count -= n_need;
    } else { // the reserve is short: hand out what is left of it, then the head of a new reservation
        const uint32_t old_base = wq.base, old_count = wq.count, more = n_need - old_count;
        const uint32_t grab = more > A.queue_grab ? more : A.queue_grab;
        const int leader = __ffsll((long long)need_mask) - 1;
        unsigned long long nb = 0;
        if ((int)lane == leader) nb = atomicAdd(&A.counters[0], (unsigned long long)grab);
        nb = __shfl(nb, leader);
        mine = rank < old_count ? (unsigned long long)old_base + rank : nb + (rank - old_count);
        wq.base = (uint32_t)(nb + more); // (the host keeps total_items + every wave's last overshoot below 2^32)
        wq.count = grab - more;
        if (nb + grab >= (unsigned long long)A.total_items) wq.drained = true;
    }
    item = (uint32_t)mine;
    return need && mine < (unsigned long long)A.total_items;
}

// Retire a finished chunk, pop a new work item for an idle slot, start the slot's next path.
template <class R, bool kAdaptive = false>
__device__ __forceinline__ void path_refill(PathState<R>& p, const TraceArgs<R>& A, uint32_t lane, WaveQueue& wq) {
    typedef typename VecOf<R>::type r4;
    if (!p.alive && p.has_item && p.s_cur == p.s_end) {
        A.partial[p.item] = r4{p.acc.x, p.acc.y, p.acc.z, R(0)};
        p.has_item = false;
    }
    {
        uint32_t got_item = 0;
        if (queue_pop<R>(A, wq, lane, !p.alive && !p.has_item && !queue_empty<R>(wq, A), got_item)) {
            p.item = got_item;
            p.has_item = true;
            const uint32_t k = place_item<R, false, kAdaptive>(A, p.item, p.px, p.py);
            chunk_bounds<R>(A, k, p.s_cur, p.s_end);
            p.acc = {R(0), R(0), R(0)};
        }
    }
    if (!p.alive && p.has_item) { // start the next path of this slot's chunk
        const unsigned long long pixel_index = (unsigned long long)p.py * A.width + p.px;
        p.g.seed_path(A.seed, pixel_index * A.spp + p.s_cur);
        camera_ray<R>(A.cam, p.g, p.px, p.py, p.o, p.d, p.time);
        p.thr = {R(1), R(1), R(1)};
        p.seg = 0;
        p.s_cur++;
        p.alive = true;
    }
}

// ---- the persistent trace kernel (flat hit list) ----------------------------------------------------------
// Work item = (pixel of this shard, chunk k of the pixel's chunk schedule: samples chunk_start[k] .. chunk_start[k+1]).
// The schedule puts the big chunks first and ends in small ones (host: chunk_schedule), so the queue's tail is made
// of short items.  Items are numbered chunk-major so
// that the 64 lanes of a wave start on 64 neighbouring pixels.  Each of a lane's NR slots owns one item at a
// time, runs its paths one after the other, adds their radiance in sample order, and stores the chunk sum to
// partial[item]; resolve_kernel adds the chunk sums of a pixel in chunk order.  The summation tree is therefore
// fixed by the chunk schedule alone — a function of (width, height, spp, chunk_spp) — not by the launch, the grid
// size, NR or the number of GPUs.
#ifndef RAYZ_FLAT_WAVES_F64
#define RAYZ_FLAT_WAVES_F64 4
#endif
template <class R, int NR> constexpr int flat_waves() { return sizeof(R) == 8 ? RAYZ_FLAT_WAVES_F64 : NR == 1 ? 4 : 3; }
#define RAYZ_TRACE_KERNEL_NAME trace_kernel
#define RAYZ_TRACE_KERNEL_ADAPTIVE false
#include "trace_kernel_flat.hpp"
#undef RAYZ_TRACE_KERNEL_NAME
#undef RAYZ_TRACE_KERNEL_ADAPTIVE
// The same text once more with the xy basis (kBasisXY: 5 packed FMAs per sphere pair in plane runs and buckets, 9 on a loose
// y-moving sphere): the host launches it for the scenes whose scan it prices lower (rayz_plane::scan_price).  A kernel of its
// own name, so that trace_kernel's code is what it was.
#define RAYZ_TRACE_KERNEL_NAME flat_xy_kernel
#define RAYZ_TRACE_KERNEL_ADAPTIVE false
#define RAYZ_TRACE_KERNEL_BASIS kBasisXY
#include "trace_kernel_flat.hpp"
#undef RAYZ_TRACE_KERNEL_NAME
#undef RAYZ_TRACE_KERNEL_ADAPTIVE
#undef RAYZ_TRACE_KERNEL_BASIS
// .. and a fourth time: the xy basis with the one-radius sets scanned by scan_sets (scan_plane_class's kSets), for scenes that
// have such sets.  A kernel of its own name for the reasons flat_xy_kernel is one (tests/test_one_radius_isa.py holds it to the limits).
#define RAYZ_TRACE_KERNEL_NAME flat_one_radius_kernel
#define RAYZ_TRACE_KERNEL_ADAPTIVE false
#define RAYZ_TRACE_KERNEL_BASIS kBasisXY
#define RAYZ_TRACE_KERNEL_SETS true
#include "trace_kernel_flat.hpp"
#undef RAYZ_TRACE_KERNEL_NAME
#undef RAYZ_TRACE_KERNEL_ADAPTIVE
#undef RAYZ_TRACE_KERNEL_BASIS
#undef RAYZ_TRACE_KERNEL_SETS
#define RAYZ_TRACE_KERNEL_NAME adaptive_pass_kernel // (an adaptive pass's kernel, DESIGN.md §4.14: the same text over the active list)
#define RAYZ_TRACE_KERNEL_ADAPTIVE true
#include "trace_kernel_flat.hpp"
#undef RAYZ_TRACE_KERNEL_NAME
#undef RAYZ_TRACE_KERNEL_ADAPTIVE
// .. and the three scan forms once more with the camera segments resolved from the pixels' primary lists: kernels
// of their own names, which the ISA tests of the kernels above do not count (tests/test_primary_lists_isa.py holds these).
// Their argument block is the trace kernels' with the lists behind it (a block of its own: a field more in TraceArgs changes
// every other kernel's code object).
template <class R> struct PrimaryTraceArgs : TraceArgs<R> {
    const uint32_t* primary; // the shard's primary lists, word j of local pixel i at [j · shard_pixels + i]
};
#define RAYZ_TRACE_KERNEL_PRIMARY true
#define RAYZ_TRACE_KERNEL_ARGS PrimaryTraceArgs<R>
#define RAYZ_TRACE_KERNEL_ADAPTIVE false
#define RAYZ_TRACE_KERNEL_NAME primary_xz_kernel
#include "trace_kernel_flat.hpp"
#undef RAYZ_TRACE_KERNEL_NAME
#define RAYZ_TRACE_KERNEL_BASIS kBasisXY
#define RAYZ_TRACE_KERNEL_NAME primary_xy_kernel
#include "trace_kernel_flat.hpp"
#undef RAYZ_TRACE_KERNEL_NAME
#define RAYZ_TRACE_KERNEL_SETS true
#define RAYZ_TRACE_KERNEL_NAME primary_one_radius_kernel
#include "trace_kernel_flat.hpp"
#undef RAYZ_TRACE_KERNEL_NAME
#undef RAYZ_TRACE_KERNEL_SETS
#undef RAYZ_TRACE_KERNEL_BASIS
#undef RAYZ_TRACE_KERNEL_ADAPTIVE
#undef RAYZ_TRACE_KERNEL_ARGS
#undef RAYZ_TRACE_KERNEL_PRIMARY
// .. and the three scan forms a third time with every listable segment resolved from the slab's cells (slab_cells.hpp, DESIGN.md
// §4.22), and a fresh path's from its pixel's primary list where the launch has lists (`primary` may be null): kernels of their own
// names again, and in a namespace of their own, rayz_dev_cells: tests/test_sparse_isa.py takes every kernel of rayz_dev it has no record
// of for a sparse-render kernel (tests/test_slab_cells_isa.py holds these).  Their argument block is the primary kernels' with the grid
// and the table behind it.
template <class R> struct CellsTraceArgs : PrimaryTraceArgs<R> {
    rayz_cells::CellGrid grid;
    const uint32_t* cells; // [kTableHead outlier slots][grid.nx · grid.nz records of kCellWords], 16-byte aligned
};
} // namespace rayz_dev (reopened below)
namespace rayz_dev_cells {
using namespace rayz_dev;
#define RAYZ_TRACE_KERNEL_CELLS true
#define RAYZ_TRACE_KERNEL_ARGS CellsTraceArgs<R>
#define RAYZ_TRACE_KERNEL_ADAPTIVE false
#define RAYZ_TRACE_KERNEL_NAME cells_xz_kernel
#include "trace_kernel_flat.hpp"
#undef RAYZ_TRACE_KERNEL_NAME
#define RAYZ_TRACE_KERNEL_BASIS kBasisXY
#define RAYZ_TRACE_KERNEL_NAME cells_xy_kernel
#include "trace_kernel_flat.hpp"
#undef RAYZ_TRACE_KERNEL_NAME
#define RAYZ_TRACE_KERNEL_SETS true
#define RAYZ_TRACE_KERNEL_NAME cells_one_radius_kernel
#include "trace_kernel_flat.hpp"
#undef RAYZ_TRACE_KERNEL_NAME
#undef RAYZ_TRACE_KERNEL_SETS
#undef RAYZ_TRACE_KERNEL_BASIS
#undef RAYZ_TRACE_KERNEL_ADAPTIVE
#undef RAYZ_TRACE_KERNEL_ARGS
#undef RAYZ_TRACE_KERNEL_CELLS
} // namespace rayz_dev_cells
namespace rayz_dev {

// ---- the primary lists' builder -----------------------------------------------------------------------------
// One lane per local pixel of the shard (place_item's numbering, rows as they come): every sphere of the pool, by its slot, through
// rayz_primary::beam_may_hit in f64; the slots that pass are the pixel's list, kNoList its count when more than kListK do.  The
// loop is wave-uniform (the sphere's record arrives through scalar loads); `real_slots` names the slots that hold a sphere, in
// slot order: a pad's record is no sphere and may never become a candidate.
struct PrimaryArgs {
    rayz_primary::BeamCamera cam;
    const d4* slot64;
    const uint32_t* real_slots;
    uint32_t* lists; // [(kListK + 1) · shard_pixels]
    uint32_t n_real, width, tile_rows, shard_index, shard_count, shard_pixels;
};
__global__ __launch_bounds__(256) void primary_lists_kernel(const PrimaryArgs A) {
    const uint32_t lane_px = blockIdx.x * 256u + threadIdx.x;
    const bool live = lane_px < A.shard_pixels;
    const uint32_t lp = live ? lane_px : A.shard_pixels - 1u; // (the last block's spare lanes repeat the last pixel and store nothing)
    const uint32_t lr = lp / A.width, px = lp - lr * A.width;
    const uint32_t tl = lr / A.tile_rows, within = lr - tl * A.tile_rows;
    const uint32_t py = (tl * A.shard_count + A.shard_index) * A.tile_rows + within;
    const rayz_primary::PixelBeam beam = rayz_primary::pixel_beam(A.cam, px, py);
    uint32_t n = 0;
    for (uint32_t i = 0; i < A.n_real; ++i) {
        const uint32_t slot = A.real_slots[i];
        const d4 c4 = A.slot64[2 * slot], v4 = A.slot64[2 * slot + 1];
        const double c[3] = {c4.x, c4.y, c4.z}, v[3] = {v4.x, v4.y, v4.z};
        if (rayz_primary::beam_may_hit(beam, c, v, __builtin_sqrt(c4.w))) {
            if (live && n < rayz_primary::kListK) A.lists[(size_t)(n + 1u) * A.shard_pixels + lp] = slot;
            ++n;
        }
    }
    if (live) A.lists[lp] = n <= rayz_primary::kListK ? n : rayz_primary::kNoList;
}

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

// ---- persistent trace kernel, BVH traversal ------------------------------------------------------
// Same work items, queue and summation tree as trace_kernel.  Traversal is per lane, so the wave's lanes want
// different code at different times; each ROUND therefore runs three convergent phases instead of one divergent
// step: (N) box steps until most lanes are parked at a leaf, (L) the parked leaves' reject tests together,
// (C) the parked sphere candidates' f64 roots together.  The nearest hit (with its tie rule) does not depend on
// the order in which hittables are examined, so this scheduling changes no result — only how much pruning the
// shrinking tbest achieves.  When too few lanes still have nodes to visit, the finished lanes are shaded and
// refilled (ray regeneration) while the others keep their query state and resume.
#ifndef RAYZ_STAT_SPILL
#define RAYZ_STAT_SPILL 0x7fffffffu // tests build with a small value to exercise the spill
#endif
constexpr int kBvhKeepActive = 20;   // rounds continue while at least this many lanes still walk
constexpr int kBvhKeepStepping = 18; // phase N continues while at least this many lanes can take a box step
                                     // (defaults; TraceArgs::bvh_keep carries the values in use)

// Waves per SIMD the register allocation aims at: 4 (128 VGPRs, nothing spilled).  At 5 (96 VGPRs) the kernel spills 54
// VGPRs into the box-step loop and is 8 % slower; the box steps are issue-bound, not latency-bound (profiles/r02), so the
// fifth wave buys nothing.
#ifndef RAYZ_BVH_WAVES
#define RAYZ_BVH_WAVES 4
#endif
#ifndef RAYZ_BVH_WAVES_F64 // the f64 kernel fits 128 VGPRs too since its box walk and its reject tests run in f32 (it needed
#define RAYZ_BVH_WAVES_F64 4 // 151 and ran 3 waves per SIMD before: +13 % from the fourth)
#endif
template <class R> constexpr int bvh_waves() { return sizeof(R) == 8 ? RAYZ_BVH_WAVES_F64 : RAYZ_BVH_WAVES; }
#define RAYZ_TRACE_KERNEL_NAME trace_kernel_bvh
#define RAYZ_TRACE_KERNEL_ADAPTIVE false
#include "trace_kernel_bvh.hpp"
#undef RAYZ_TRACE_KERNEL_NAME
#undef RAYZ_TRACE_KERNEL_ADAPTIVE
#define RAYZ_TRACE_KERNEL_NAME adaptive_pass_kernel_bvh // (an adaptive pass's kernel, DESIGN.md §4.14: the same text over the active list)
#define RAYZ_TRACE_KERNEL_ADAPTIVE true
#include "trace_kernel_bvh.hpp"
#undef RAYZ_TRACE_KERNEL_NAME
#undef RAYZ_TRACE_KERNEL_ADAPTIVE

// The retired experiment kernels (two paths per lane; walker / shader waves — DESIGN.md §6) live in experiments/: they need the
// walk above and nothing below needs them.  bench.py ties a committed profile to a build by hashing rayz_device.hpp, rayz_hip.hip,
// bvh_build.hpp and include/rayz_hip.h, so every line a product trace kernel is compiled from, and everything that decides what it
// is launched with (scene upload, chunk schedule, LDS layout, the trace launch itself: rayz_hip.hip), has to stay in those four — do
// not split product DEVICE code or the trace launch into further headers.  Outside them may live experiment code, the host
// library's base (host_base.hpp) and the host code of features that only use the trace launch (progressive.hpp, multi_device.hpp,
// query.hpp, denoiser.hpp, known_answers.hpp).
#ifdef RAYZ_EXPERIMENTS
#include "experiments/bvh2_kernel.hpp"
#include "experiments/bvhx_kernel.hpp"
#endif

// ---- pixel = (Σ_chunks partial) · (1/spp), chunk order: src/renderer.zig:94-95 ---------------------
template <class R>
__global__ __launch_bounds__(256) void resolve_kernel(const typename VecOf<R>::type* __restrict__ partial,
                                                      R* __restrict__ out, uint32_t shard_pixels,
                                                      uint32_t chunks_per_px, uint32_t spp) {
    typedef typename VecOf<R>::type r4;
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= shard_pixels) return;
    R x = 0, y = 0, z = 0;
    for (uint32_t k = 0; k < chunks_per_px; ++k) {
        const r4 p = partial[(size_t)k * shard_pixels + lp];
        x = x + p.x;
        y = y + p.y;
        z = z + p.z;
    }
    const R inv = R(1) / (R)spp;
    out[3 * (size_t)lp + 0] = x * inv;
    out[3 * (size_t)lp + 1] = y * inv;
    out[3 * (size_t)lp + 2] = z * inv;
}

// ---- progressive passes: acc = acc + partial[k] for the pass's chunks in chunk order; preview = acc · (1/samples_done) ------
// resolve_kernel's loop cut at the passes' boundaries: the same additions in the same order, the running sum kept in `acc`
// between passes (stored in R, so nothing is rounded that resolve_kernel keeps in a register).  After the last pass acc holds
// resolve_kernel's x bit for bit and the preview (samples_done = spp) is its pixel.  `first`: the pass that starts at chunk 0
// begins from +0, as resolve_kernel does, without reading acc.  A streaming kernel: one 16-byte (f32) load per chunk and pixel.
template <class R>
__global__ __launch_bounds__(256) void accumulate_kernel(const typename VecOf<R>::type* __restrict__ partial,
                                                         typename VecOf<R>::type* __restrict__ acc, R* __restrict__ out,
                                                         uint32_t shard_pixels, uint32_t chunks, uint32_t samples_done,
                                                         uint32_t first) {
    typedef typename VecOf<R>::type r4;
    const uint32_t lp = blockIdx.x * blockDim.x + threadIdx.x;
    if (lp >= shard_pixels) return;
    R x = 0, y = 0, z = 0;
    if (!first) {
        const r4 a = acc[lp];
        x = a.x, y = a.y, z = a.z;
    }
    for (uint32_t k = 0; k < chunks; ++k) {
        const r4 p = partial[(size_t)k * shard_pixels + lp];
        x = x + p.x;
        y = y + p.y;
        z = z + p.z;
    }
    acc[lp] = r4{x, y, z, R(0)};
    if (out) {
        const R inv = R(1) / (R)samples_done;
        out[3 * (size_t)lp + 0] = x * inv;
        out[3 * (size_t)lp + 1] = y * inv;
        out[3 * (size_t)lp + 2] = z * inv;
    }
}

// ---- `writePPM`'s per-pixel transform, src/image.zig:35-38 + src/vec.zig:79-93 -------------------
__global__ __launch_bounds__(256) void tonemap_kernel(const float* __restrict__ rgb, uint8_t* __restrict__ out,
                                                      size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // in f64, as writePPM computes it on the widened pixel: bit-identical to the host writer
    const double v = (double)rgb[i];
    double s = v > 0.0 ? __builtin_sqrt(v) : 0.0;
    s = s > 0.0 ? s : 0.0; // utils.max(x, low)
    s = s < 1.0 ? s : 1.0; // utils.min(.., high)
    out[i] = (uint8_t)(s * 255.0);
}

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
