// device_types.hpp — what the device code of the render path is written in terms of: the address-space macros and vector
// typedefs, the scan's group sizes, the device-resident scene (DevScene: the HBM layout of the scan streams, the shading tables and
// the BVH), the camera (DevCamera) and the trace kernels' argument block (TraceArgs).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "plane_runs.hpp"

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

} // namespace rayz_dev
