/*
 * rayz_hip.h — C ABI of the MI355X (gfx950) render path that replaces the loop
 * nest of rayz's `Tracer.render()`.
 *
 * Every entry point cites the reference interface it stands in for
 * (file:line into jlucier/rayz @ 2025-07-25).  The reference has no FFI of its
 * own: its boundary is the single Zig method `Tracer.render`
 * (src/renderer.zig:72-101).  A Zig caller copies its `MemPool` lists and its
 * `Camera` field by field into the `extern struct`-compatible PODs below
 * (Zig `struct`/`union(enum)` have no defined layout, so `items.ptr` cannot be
 * passed directly), calls `rayz_hip_render`, and widens the returned f32 RGB
 * into `img.pixels`.  See INTEGRATION.md for the Zig stub.
 *
 * Plain pointers and sizes only; no C++ types, exceptions or aborts cross this
 * boundary.  All functions return RAYZ_OK (0) or a negative RayzStatus and
 * leave a message retrievable through rayz_hip_last_error().
 */
#ifndef RAYZ_HIP_H
#define RAYZ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RAYZ_HIP_ABI_VERSION 5u /* 2: RayzTriangle, shard fields; 3: RAYZ_TRAVERSAL_AUTO; 4: per-scene devices,
                                   rayz_hip_multi_* (several GPUs behind one call), rayz_hip_kat, chunk_spp auto;
                                   5: rayz_hip_debug_set (the library reads no environment variable),
                                   rayz_hip_multi_device_stats / _timing, RAYZ_GATHER_ALLOW_DUPLICATE_DEVICES */
#define RAYZ_DEFAULT_TILE_ROWS 8u /* what RayzRenderParams.tile_rows = 0 means (see there) */
#define RAYZ_MAX_DEVICES 64

typedef enum RayzStatus {
    RAYZ_OK = 0,
    RAYZ_ERR_BAD_ARG = -1,   /* null pointer, zero size, index out of range, bad enum */
    RAYZ_ERR_HIP = -2,       /* a HIP runtime call failed; text in rayz_hip_last_error() */
    RAYZ_ERR_OOM = -3,       /* host or device allocation failed */
    RAYZ_ERR_NO_DEVICE = -4, /* no usable gfx950 device / library not initialised */
    RAYZ_ERR_STATE = -5      /* bad handle, call order */
} RayzStatus;

/* Tag order follows `Texture = union(enum){ checker, solid }`, src/material.zig:41-44. */
typedef enum RayzTextureKind { RAYZ_TEX_CHECKER = 0, RAYZ_TEX_SOLID = 1 } RayzTextureKind;
/* `Material = union(enum){ diffuse, metallic, dielectric }`, src/material.zig:162-165. */
typedef enum RayzMaterialKind {
    RAYZ_MAT_DIFFUSE = 0,
    RAYZ_MAT_METALLIC = 1,
    RAYZ_MAT_DIELECTRIC = 2
} RayzMaterialKind;
/* `DiffuseScatterMethod`, src/material.zig:67-71 (default HEMISPHERE, :74). */
typedef enum RayzDiffuseMethod {
    RAYZ_DIFFUSE_UNIT_SPHERE = 0,
    RAYZ_DIFFUSE_UNIT_SPHERE_SURFACE = 1,
    RAYZ_DIFFUSE_HEMISPHERE = 2
} RayzDiffuseMethod;

typedef enum RayzPrecision {
    RAYZ_PRECISION_F32 = 0, /* the kernel arithmetic of DESIGN.md §4 (tmin 1e-3 recommended) */
    RAYZ_PRECISION_F64 = 1  /* fidelity mode: the reference's own scalar type, src/vec.zig:4-8 */
} RayzPrecision;

typedef enum RayzTraversal {
    RAYZ_TRAVERSAL_LINEAR = 0, /* flat hit list: every sphere tested per segment (north star) */
    RAYZ_TRAVERSAL_BVH = 1,    /* the reference's accelerator, src/hit.zig:101-217 */
    RAYZ_TRAVERSAL_AUTO = 2    /* flat list up to RAYZ_AUTO_BVH_MIN hittables, BVH above (same image either way) */
} RayzTraversal;
#define RAYZ_AUTO_BVH_MIN 160u /* measured crossover on MI355X: tools/crossover.py, profiles/r02/crossover.log */

/* One entry of `MemPool.textures` (src/ecs.zig:26): SolidTexture src/material.zig:19-25 or
 * CheckerTexture src/material.zig:27-39.  `even`/`odd` are TextureHandle.idx values. */
typedef struct RayzTexture {
    uint32_t kind; /* RayzTextureKind */
    uint32_t even; /* checker only */
    uint32_t odd;  /* checker only */
    uint32_t _pad;
    double scale;    /* checker only */
    double color[3]; /* solid only */
} RayzTexture;

/* One entry of `MemPool.materials` (src/ecs.zig:25): DiffuseMaterial src/material.zig:73-75,
 * MetallicMaterial :104-106, DielectricMaterial :134-135. */
typedef struct RayzMaterial {
    uint32_t kind;    /* RayzMaterialKind */
    uint32_t texture; /* TextureHandle.idx (diffuse, metallic) */
    uint32_t method;  /* RayzDiffuseMethod (diffuse) */
    uint32_t _pad;
    double param;     /* metallic: fuzz; dielectric: refractive_index */
} RayzMaterial;

/* One entry of `MemPool.spheres` (src/ecs.zig:24): `Sphere{center: Ray, radius, material}`,
 * src/geom.zig:11-14.  `center` = center.origin, `velocity` = center.dir (center.time unused). */
typedef struct RayzSphere {
    double center[3];
    double velocity[3];
    double radius;
    uint32_t material; /* MaterialHandle.idx */
    uint32_t _pad;
} RayzSphere;

/* A triangle hittable.  BUILD-DEFINED: the reference's geom.zig holds only `Sphere` (src/geom.zig:11-67);
 * BASELINE.json's config 5 asks for a triangle path, so this primitive is fitted to the `Hittable` / `Hit`
 * contract (src/hit.zig:8-42): two-sided, nearest root in [tmin, tmax], geometric normal flipped to face the
 * ray by `Hit.init`, stationary.  Its results are parity-unpinned (no reference code or test exists). */
typedef struct RayzTriangle {
    double v0[3];
    double v1[3];
    double v2[3];
    uint32_t material; /* MaterialHandle.idx */
    uint32_t _pad;
} RayzTriangle;

/* The `MemPool` lists (src/ecs.zig:22-27) plus the build-defined triangle list, borrowed for the duration of
 * the call.  Hittables are numbered spheres first, then triangles (the order `initHittables` would append
 * them, src/ecs.zig:43-51). */
typedef struct RayzSceneDesc {
    const RayzSphere* spheres;
    const RayzMaterial* materials;
    const RayzTexture* textures;
    uint32_t n_spheres;
    uint32_t n_materials;
    uint32_t n_textures;
    uint32_t n_triangles;
    const RayzTriangle* triangles;
} RayzSceneDesc;

/* The fields of `Camera` AFTER `Camera.init` (src/camera.zig:9-16): results, not look-at params. */
typedef struct RayzCameraDesc {
    double look_from[3];
    double px_du[3];
    double px_dv[3];
    double px_origin[3];
    double defocus_u[3];
    double defocus_v[3];
    uint32_t defocus; /* bool */
    uint32_t _pad;
} RayzCameraDesc;

/* `Tracer` fields that steer render() (src/renderer.zig:18-28) plus what the reference lacks:
 * a settable seed (it seeds from getrandom, :55-59), an explicit tmin (hard-coded 1e-10 at :107),
 * the precision/traversal selectors and the row-tile shard for multi-GPU. */
typedef struct RayzRenderParams {
    uint32_t width;  /* img.w, src/image.zig:6 */
    uint32_t height; /* img.h, src/image.zig:5 */
    uint32_t samples_per_px; /* src/renderer.zig:24 */
    uint32_t max_bounces;    /* src/renderer.zig:23 */
    uint64_t seed;           /* key of the per-(pixel,sample) PCG32 streams */
    double tmin;             /* src/renderer.zig:107 passes 1e-10 */
    uint32_t precision;      /* RayzPrecision */
    uint32_t traversal;      /* RayzTraversal */
    uint32_t chunk_spp;      /* samples summed per work item; 0 = the automatic schedule (rayz_hip_chunk_schedule);
                                part of the image's definition (fixes the f32 summation tree) */
    uint32_t tile_rows;      /* rows per shard tile; 0 = RAYZ_DEFAULT_TILE_ROWS (8) in EVERY entry point, single- and multi-device
                                alike.  Why 8: the BVH kernel deals its work as 8x8 pixel tiles of a shard's LOCAL rows, which are 8
                                consecutive image rows only with 8-row shard tiles; measured on an 8-way deal (every shard timed on one
                                GPU, profiles/r04/multi/tile_rows_ab.log): +8.6 % at 1920x1080 (rows 128..136 per rank) and +1.7 % at
                                3840x2160 against 1-row interleave, whose perfect row balance (135 each) does not make up for tiles
                                that span 57 image rows.  Irrelevant when shard_count <= 1 */
    uint32_t shard_index;    /* this call renders rows with (row / tile_rows) % shard_count == shard_index.  (Dealing the tiles in alternating
                                direction per band of shard_count — so that no shard's rows lie systematically lower in the frame, where paths
                                are longer — was measured in round 4 and NOT adopted: 7.09x instead of 6.91x for the flat list on 8 shards, but
                                6.99x instead of 7.17x through the BVH and worse at 2 and 4 shards, where it pairs adjacent tiles:
                                profiles/r04/multi/predicted_scaling_*.log) */
    uint32_t shard_count;    /* 0 or 1 = whole image */
} RayzRenderParams;

/* What `render()` returns (primary rays, src/renderer.zig:90,100) plus the counts the roofline needs. */
typedef struct RayzRenderStats {
    uint64_t primary_rays; /* rows_in_shard * width * samples_per_px */
    uint64_t segments;     /* findHit calls: one per ray segment, src/renderer.zig:107 */
    uint64_t sphere_tests; /* primitive tests: Sphere.hitInner evaluations (src/geom.zig:38-66) + triangle tests.  BVH: counted by
                              the kernel (leaf entries examined).  Flat list: DERIVED, segments x hittables — every segment scans
                              the whole list, so the kernel counts segments only */
    uint64_t node_tests;   /* AABB.hit evaluations (BVH traversal only), src/hit.zig:70-98 */
    double kernel_ms;      /* HIP-event time of the trace kernel(s) of the last render on this scene */
} RayzRenderStats;

typedef struct RayzScene RayzScene; /* opaque: device-resident scene + workspace */

/* Library / device lifetime.  rayz_hip_init(device) creates the context of that HIP ordinal (its stream, CU count;
 * gfx950 only) and makes it the DEFAULT device: the one the entry points without a device argument use.  Idempotent;
 * calling it for a second ordinal adds a context and moves the default, it does not re-target existing scenes —
 * a scene stays on the device it was bound to.  Every entry point selects its device itself and restores the
 * calling thread's current HIP device on return.  rayz_hip_shutdown destroys all contexts (scenes must be
 * destroyed first; a scene destroyed later still frees its memory). */
int rayz_hip_init(int device);
void rayz_hip_shutdown(void);
const char* rayz_hip_last_error(void);
uint32_t rayz_hip_abi_version(void);

/* Measurement knobs.  They change how the work is SCHEDULED or which (equivalent) tree the GPU walks — never an image —
 * and exist for the sweep tools under tools/ and for the tests that hold the kernels against each other.  Process-wide;
 * value < 0 restores the built-in default; takes effect for renders (BVH_PEEL / BVH_TOP: scenes) started afterwards.
 * The library reads NO environment variable. */
typedef enum RayzDebugKnob {
    RAYZ_DEBUG_QUEUE_GRAB = 0, /* work items a wave reserves per atomic on the queue head (default 64) */
    RAYZ_DEBUG_BVH_KEEP = 1,   /* one-path BVH kernel: keep_active | keep_stepping << 8 */
    RAYZ_DEBUG_BVH_PEEL = 2,   /* 0: walk the reference's full tree (oversized hittables stay in it) */
    RAYZ_DEBUG_BVH_TOP = 3,    /* cap on the inner-node records of the tree's top kept in LDS (default: what fits beside the stacks) */
    RAYZ_DEBUG_BVH_KERNEL = 4, /* f32 BVH renders: 1 = one path per lane (trace_kernel_bvh, default; the only one in the product library);
                                  -DRAYZ_EXPERIMENTS builds: 2 = two paths per lane (trace_kernel_bvh2), 3 = walker / shader waves (trace_kernel_bvhx) */
    RAYZ_DEBUG_BVH2_KEEP = 5,  /* two-path BVH kernel: service | blocked << 8 | swap << 16 | keep_stepping << 24 */
    RAYZ_DEBUG_LDS_PAD = 6,    /* BVH kernels: unused bytes added to the workgroup's LDS request (occupancy experiments) */
    RAYZ_DEBUG_BVH_TOP_ORDER = 7, /* which inner nodes the LDS top holds: 0 = by box surface area from the root (default), 1 = breadth-first */
    RAYZ_DEBUG_BVH_NODES = 8,     /* node record format of trees built from now on: 0 = by tree size (default), 1 = f32 planes (64 B), 2 = 16-bit plane indices (32 B) */
    RAYZ_DEBUG_BVH_SPLIT = 9,     /* how trees built from now on split a node: 0 = surface-area heuristic (default), 1 = the reference's median split */
    RAYZ_DEBUG_BVHX = 10,         /* exchange kernel (RAYZ_DEBUG_BVH_KERNEL = 3, -DRAYZ_EXPERIMENTS builds only): slots per walker wave | exchange threshold << 8 |
                                     shader's minimum batch << 16 | its patience << 24 | its priority << 32 */
    RAYZ_DEBUG_CHUNK_CAP = 11,    /* -DRAYZ_EXPERIMENTS builds only, refused otherwise — it CHANGES the image's summation tree (the one knob that
                                     does; tools/chunk_cap_sweep.py): largest chunk of the automatic schedule */
    RAYZ_DEBUG_DENOISE_LDS_STRIDE = 12, /* denoiser: the largest stride whose level stages tile + halo in LDS — 0 (every level reads its taps from
                                     global memory), 1, 2 or 4; the same image either way */
    RAYZ_DEBUG_KNOBS = 13
} RayzDebugKnob;
int rayz_hip_debug_set(uint32_t knob, long long value);

/* Number of rows the shard described by `p` owns (= rows of the compact output). */
uint32_t rayz_hip_shard_rows(const RayzRenderParams* p);

/* The chunk schedule the render of `p` will use — which consecutive samples of a pixel are summed by one work item;
 * the chunk sums are then added in chunk order (it fixes the f32 summation tree, so it is part of the
 * image's definition; it depends on width, height, samples_per_px and chunk_spp only, never on the shard fields).
 * Returns the number of chunks n; if `starts` is not NULL, fills starts[0..min(n, capacity-1)] with the first sample
 * of each chunk and, last, samples_per_px.  chunk_spp = 0 selects the automatic schedule (uniform 16 for small
 * renders; 256, 256, .., 128, 64, 32, 16, 16 for large ones). */
uint32_t rayz_hip_chunk_schedule(const RayzRenderParams* p, uint32_t* starts, uint32_t capacity);

/* Replaces src/renderer.zig:76-78 (initHittables + BVH build) and what follows it: validates the
 * handles (RAYZ_ERR_BAD_ARG for an index out of range, a checker chain that contains a cycle or nests deeper than
 * 8 lookups — the reference recurses without a limit, src/material.zig:36-37, the device walks a bounded loop),
 * lays the pool out in HBM and (for BVH traversal) builds the reference's BVH on the host.
 * rayz_hip_scene_create binds the scene to the default device at its first render; _create_on binds it to
 * `device` now (creating that device's context if needed).  One render in flight per scene. */
int rayz_hip_scene_create(const RayzSceneDesc* scene, RayzScene** out);
int rayz_hip_scene_create_on(int device, const RayzSceneDesc* scene, RayzScene** out);
int rayz_hip_scene_destroy(RayzScene* scene);

/* The BVH `render()` would build (src/renderer.zig:76-78 -> src/hit.zig:130-161), flattened in depth-first
 * pre-order with skip links as the GPU traverses it.  Host only (no device needed).  Call once with every array
 * NULL to get *n_nodes, then with arrays of n_nodes (boxes: 6 doubles per node, lo then hi; skip/first/count:
 * one u32 per node; order: n_spheres + n_triangles hittable indices in leaf order).  count == 0 marks an inner node. */
int rayz_hip_scene_bvh(RayzScene* scene, uint32_t* n_nodes, uint32_t* depth, double* boxes, uint32_t* skip,
                       uint32_t* first, uint32_t* count, uint32_t* order);

/* Replaces the loop nest src/renderer.zig:80-97.  Asynchronous on `hip_stream` (a hipStream_t, or
 * NULL for the library's own stream); `d_rgb_out` is DEVICE memory, rows_in_shard*width*3 floats,
 * row-major packed RGB, linear radiance means as `img.pixels` holds them (src/renderer.zig:94-95;
 * no gamma or clamp, those live in writePPM, src/image.zig:29-41). */
int rayz_hip_render_device(RayzScene* scene, const RayzCameraDesc* camera, const RayzRenderParams* params,
                           float* d_rgb_out, void* hip_stream);

/* Same, f64 output (precision F64): rows_in_shard*width*3 doubles. */
int rayz_hip_render_device_f64(RayzScene* scene, const RayzCameraDesc* camera, const RayzRenderParams* params,
                               double* d_rgb_out, void* hip_stream);

/* The basis of the flat list's reject test.  Both forms find the same candidates up to roundings the filter's
 * pad covers, and the f64 narrow phase decides: the image is the same, bit for bit.  XZ (e1 in the xz-plane) tests a sphere
 * pair of a plane run or speed bucket in 6 packed FMAs and a loose y-moving one in 8; XY (e1 in the xy-plane) in 5 and 9.
 * AUTO prices one scan of the scene under both from its slot counts and takes XY only where it is strictly cheaper.  The
 * form applies to the one-shot and progressive flat-list renders; adaptive passes, ray queries and the BVH kernels keep XZ.
 * ONE_RADIUS is XY with the scene's one-radius sets scanned in a loop of their own: members of a static plane run or of a speed
 * bucket whose radii lie within r_min / 16 of each other are tested with the largest of them, held once per set, in blocks of
 * cx and cz alone.  A scene without such sets renders under it as under XY.  AUTO takes it wherever it takes XY and the scene's
 * sets hold at least 1,024 spheres (fewer do not pay for the set tables' loads); XY itself never does.
 * _get returns the form the next flat-list render uses, never AUTO (host only: no device needed).  Default AUTO. */
typedef enum RayzScanForm { RAYZ_SCAN_FORM_AUTO = 0, RAYZ_SCAN_FORM_XZ = 1, RAYZ_SCAN_FORM_XY = 2, RAYZ_SCAN_FORM_ONE_RADIUS = 3 } RayzScanForm;
int rayz_hip_scene_set_scan_form(RayzScene* scene, uint32_t form);
int rayz_hip_scene_get_scan_form(RayzScene* scene, uint32_t* form);

/* Primary lists.  The spheres a pixel's camera rays can meet at all are a fact of (scene, camera, pixel): with the
 * lists ON a flat-list launch first builds every pixel's list (one brute-force f64 pass over the pool, inside the launch's events:
 * kernel_ms includes it) and resolves each path's camera segment from it, through the same f64 narrow phase that decides behind the
 * scan, instead of scanning the whole list; a pixel with more than 32 candidates keeps the scan.  The lists take 33 u32 words per pixel of the shard (274 MB at
 * 1920x1080), kept with the scene, and again with each progressive handle that uses them.  The image and the segments counter
 * are the same, bit for bit.  A second choice beside the scan form, which keeps its meaning.  It applies to one-shot and progressive
 * flat-list renders of scenes without triangles (a progressive handle builds its lists once); adaptive passes, ray queries, chain
 * calls and the BVH kernels are untouched.  AUTO takes the lists from 1,024 spheres and 128 samples per pixel of the launch on (a
 * progressive handle: of its whole schedule, which shares one build).
 * _get returns whether a flat-list launch of `samples_per_px` would use them (0 / 1; host only).  Default AUTO. */
typedef enum RayzPrimaryLists { RAYZ_PRIMARY_LISTS_AUTO = 0, RAYZ_PRIMARY_LISTS_OFF = 1, RAYZ_PRIMARY_LISTS_ON = 2 } RayzPrimaryLists;
int rayz_hip_scene_set_primary_lists(RayzScene* scene, uint32_t mode);
int rayz_hip_scene_get_primary_lists(RayzScene* scene, uint32_t samples_per_px, uint32_t* on);

/* Cell lists.  The spheres that do not move in x or z and are no wider than a cell of a grid laid over their
 * centres (the MEMBERS) live between two heights for the whole shutter.  With the cells ON a flat-list render asks, per segment,
 * under which cells the ray's stretch between those heights runs; if they are at most 12, it resolves the segment from those cells'
 * spheres and the scene's other hittables (the OUTLIERS, at most 8), through the same f64 narrow phase that decides behind the scan,
 * instead of scanning the whole list.  A wave scans as before once fewer than 16 of its lanes hold such a segment.  The image and
 * the segments counter are the same, bit for bit.  The table is a fact of the scene alone (4 u32 words per cell, built with the
 * scene's slots, nothing per launch), so there is no samples-per-pixel gate.  A third choice beside the scan form and the primary
 * lists, which keep their meaning.  It applies to one-shot and progressive flat-list renders with tmin > 0; adaptive passes, sparse
 * renders, ray queries, chain calls and the BVH kernels are untouched.  A scene with a triangle, with more than 8 outliers or
 * without a member has no cells: ON is accepted, _get reports 0 and the render scans.  AUTO takes the cells from 1,023 members on (the 32 x 32 grid of randomBouncing).
 * _get returns whether such a render would use them (0 / 1; host only).  Default AUTO. */
typedef enum RayzCellLists { RAYZ_CELL_LISTS_AUTO = 0, RAYZ_CELL_LISTS_OFF = 1, RAYZ_CELL_LISTS_ON = 2 } RayzCellLists;
int rayz_hip_scene_set_cell_lists(RayzScene* scene, uint32_t mode);
int rayz_hip_scene_get_cell_lists(RayzScene* scene, uint32_t* on);

/* Waits for the last render on `scene` and returns its counters. */
int rayz_hip_scene_sync(RayzScene* scene, RayzRenderStats* stats_or_null);

/* Blocking one-shot form of `tracer.render()` as main() calls it (src/rayz.zig:26): upload, render,
 * download into caller-owned host memory (`rgb_out`: rows_in_shard*width*3 floats). */
int rayz_hip_render(const RayzSceneDesc* scene, const RayzCameraDesc* camera, const RayzRenderParams* params,
                    float* rgb_out, RayzRenderStats* stats_or_null);
int rayz_hip_render_f64(const RayzSceneDesc* scene, const RayzCameraDesc* camera, const RayzRenderParams* params,
                        double* rgb_out, RayzRenderStats* stats_or_null);

/* ---- progressive rendering: one frame in passes --------------------------------------------------------------
 * The reference reports progress while it renders (`\rProgress: xx.xx%`, src/renderer.zig:84,98-99); these entry points
 * render the frame of rayz_hip_render_device in passes of WHOLE chunks of its chunk schedule (rayz_hip_chunk_schedule),
 * each pass adding its chunk sums to an accumulator in chunk order.  After the last pass the preview is the one-shot frame
 * bit for bit, for any partition into passes; the preview after n samples is the mean of exactly the first n samples of every
 * pixel of that frame (not a separate lower-spp render).  A pass needs chunk-sum workspace for its own chunks only.
 * A handle keeps its scene, camera and params (copied at create), its own copy of the schedule, the device accumulator
 * (rows_in_shard*width*4 values of the precision) and the cursor.  It uses the scene's workspace: one render in flight per
 * scene, as everywhere; other renders on the scene may run BETWEEN steps and change nothing of the progressive result.
 * Progressive passes leave rayz_hip_scene_sync's counters (the scene's last one-shot render) alone.  Destroy the handle
 * before its scene. */
typedef struct RayzProgressive RayzProgressive; /* opaque: scene + camera + params + device accumulator + chunk cursor */
/* Validates as rayz_hip_render_device does (either precision); binds the scene to the default device if it is not bound. */
int rayz_hip_progressive_create(RayzScene* scene, const RayzCameraDesc* camera, const RayzRenderParams* params,
                                RayzProgressive** out);
/* One pass, asynchronous on `hip_stream` (NULL: the library's stream): the fewest whole chunks from the cursor that add at
 * least `min_samples` samples — at least one chunk (min_samples = 0), at most the rest of the frame (UINT32_MAX).  If
 * `d_preview_or_null` is not NULL it receives the frame so far (DEVICE memory, rows_in_shard*width*3 values, as
 * rayz_hip_render_device writes).  The entry must match params.precision (RAYZ_ERR_BAD_ARG); stepping a finished render
 * is RAYZ_ERR_STATE. */
int rayz_hip_progressive_step(RayzProgressive* pr, uint32_t min_samples, float* d_preview_or_null, void* hip_stream);
int rayz_hip_progressive_step_f64(RayzProgressive* pr, uint32_t min_samples, double* d_preview_or_null, void* hip_stream);
/* Samples per pixel and chunks done so far, and the schedule's chunk count: host state, no wait.  `total_or_null` waits for
 * the passes so far and sums their counters (primary_rays, segments, sphere_tests, node_tests, kernel_ms).  Any pointer may
 * be NULL. */
int rayz_hip_progressive_info(const RayzProgressive* pr, uint32_t* samples_done, uint32_t* chunks_done,
                              uint32_t* n_chunks, RayzRenderStats* total_or_null);
int rayz_hip_progressive_destroy(RayzProgressive* pr);

/* ---- noise estimate: "is this pixel done?" -----------------------------------------------------------------------------
 * BUILD-DEFINED (the reference reports progress towards a sample count only, src/renderer.zig:84,98-99).  A progressive handle
 * that TRACKS noise keeps, beside its accumulator, the second moment of every pixel's chunk sums (three f64 per pixel in a 32-byte
 * record, folded in chunk order, so the same bits for any partition into passes).  The chunk sums of a pixel are independent sums
 * of iid samples, so their spread is an unbiased estimate of the variance of the pixel's mean: `var`, channels summed.  `rel2` is
 * var / max(|mean|^2, mean_floor^2) — the squared relative error of the pixel — and a pixel is UNCONVERGED iff
 * !(rel2 <= rel_error^2), so a NaN counts as unconverged.  Before the second chunk there is no estimate: var = rel2 = +inf.
 * With few chunks the estimate itself is noisy (K - 1 degrees of freedom).  The arithmetic is a contract, DESIGN.md §4.12 (f64,
 * + - x /, comparisons; no FMA, no sqrt), restated bit for bit by tests/noise_ref.py.  Tracking changes no image.  Added in ABI 5
 * (additive: no existing symbol changed). */
#define RAYZ_NOISE_DEFAULT_REL_ERROR 0.05  /* parameters, not contract */
#define RAYZ_NOISE_DEFAULT_MEAN_FLOOR 0.02 /* pixels darker than this (|mean RGB|) are held to the absolute error rel_error x mean_floor */
typedef struct RayzNoiseParams {
    double rel_error;  /* > 0 (and its square > 0): the relative standard error of the pixel mean at which a pixel counts as converged */
    double mean_floor; /* > 0 (and its square > 0) */
} RayzNoiseParams;

typedef struct RayzNoiseSummary {
    uint64_t pixels;      /* pixels of the handle's shard */
    uint64_t unconverged; /* of those, pixels with !(rel2 <= rel_error^2) */
    double max_rel2;      /* the largest rel2 (a NaN anywhere surfaces here as a NaN; +inf before the second chunk) */
    double mean_var;      /* (sum of the finite var) / pixels; 0 for an empty shard */
    uint32_t samples_done;/* N: samples per pixel the estimate covers */
    uint32_t chunks_done; /* K: chunks the estimate covers */
} RayzNoiseSummary;

/* Makes `pr` a tracked handle: allocates the moment state (rows_in_shard*width*32 bytes).  Only before the first step
 * (RAYZ_ERR_STATE afterwards); a second call before the first step is RAYZ_OK and does nothing.  An untracked handle runs
 * exactly what it ran before this entry point existed. */
int rayz_hip_progressive_track_noise(RayzProgressive* pr);
/* Evaluates the estimate for the samples done so far.  `d_var_or_null`, `d_rel2_or_null`: DEVICE memory, rows_in_shard*width
 * floats each (the f64 values rounded once), written asynchronously on `hip_stream` (NULL: the library's stream), which the call
 * orders after the handle's last pass on the device.  With `summary_or_null` the call waits for the few summary values and fills
 * it; without it nothing blocks: the outputs are complete once `hip_stream` has been waited for (rayz_hip_progressive_info with
 * `total_or_null` also waits for the handle's last evaluation, as does destroying the handle).  p_or_null == NULL: the defaults.  RAYZ_ERR_BAD_ARG (checked first, before any device work): a
 * rel_error or mean_floor that is not positive (NaN included) or whose square is not; RAYZ_ERR_STATE: an untracked handle. */
int rayz_hip_progressive_noise(RayzProgressive* pr, const RayzNoiseParams* p_or_null, float* d_var_or_null, float* d_rel2_or_null,
                               RayzNoiseSummary* summary_or_null, void* hip_stream);
/* The variance of the pixel mean PER CHANNEL, for a consumer that filters each channel on its own scale (the guided denoiser,
 * rayz_hip_denoiser_run_guided): `d_var_rgb`, DEVICE memory, rows_in_shard*width*3 floats packed as frames are, receives
 * var_ch = D_ch / ((K - 1) * N) with DESIGN.md §4.12's D_ch (its clamp at 0 included), computed in f64 and rounded once; before the
 * second chunk all three are +inf.  Their sum is `var` up to the order of the roundings.  Asynchronous on `hip_stream` and ordered
 * as rayz_hip_progressive_noise is; nothing blocks.  RAYZ_ERR_STATE: an untracked handle; RAYZ_ERR_BAD_ARG: a null buffer. */
int rayz_hip_progressive_noise_rgb(RayzProgressive* pr, float* d_var_rgb, void* hip_stream);
/* The moment state itself, for tests and tools: rows_in_shard*width*4 doubles {Q_r, Q_g, Q_b, 0} copied to DEVICE memory `d_q`
 * on `hip_stream`, ordered after the handle's last pass.  Blocks until the copy is done. */
int rayz_hip_progressive_noise_state(RayzProgressive* pr, double* d_q, void* hip_stream);
/* Render until converged: steps a tracked handle with `min_samples_per_pass` (as rayz_hip_progressive_step) and evaluates after
 * every pass, until unconverged <= max_unconverged_fraction * pixels or the schedule ends — both are RAYZ_OK;
 * last_summary_or_null->chunks_done (against rayz_hip_progressive_info's n_chunks) and ->unconverged tell which.  It stops at
 * pass boundaries only, so the frame in `d_preview_or_null` is the mean of the first samples_done samples of every pixel, and
 * the one-shot frame bit for bit once the schedule has ended.  Blocks.  max_unconverged_fraction must lie in [0, 1].  A shard
 * without pixels has nothing unconverged: it stops after its first pass. */
int rayz_hip_progressive_run_until(RayzProgressive* pr, const RayzNoiseParams* p_or_null, double max_unconverged_fraction,
                                   uint32_t min_samples_per_pass, float* d_preview_or_null, RayzNoiseSummary* last_summary_or_null,
                                   void* hip_stream);
int rayz_hip_progressive_run_until_f64(RayzProgressive* pr, const RayzNoiseParams* p_or_null, double max_unconverged_fraction,
                                       uint32_t min_samples_per_pass, double* d_preview_or_null, RayzNoiseSummary* last_summary_or_null,
                                       void* hip_stream);
/* Known answers, as rayz_hip_kat: runs the two kernels on caller chunk sums — HOST buffers, chunk_sums[(k*n_pixels + i)*3 + ch]
 * (narrowed to `precision` as a scene is), chunk_sizes[k] > 0 samples in chunk k — as a tracked handle would have folded them
 * (chunk 0 as a first pass, the rest as a second), on the default device; no scene needed.  Outputs (HOST, each optional):
 * q_out n_pixels*3, var_out and rel2_out n_pixels doubles (the f64 values), the summary as rayz_hip_progressive_noise fills it. */
int rayz_hip_noise_kat(uint32_t precision, const double* chunk_sums, const uint32_t* chunk_sizes, uint32_t n_pixels,
                       uint32_t n_chunks, const RayzNoiseParams* p_or_null, double* q_out, double* var_out, double* rel2_out,
                       RayzNoiseSummary* summary_or_null);

/* ---- adaptive passes: stop tracing the pixels the estimate calls done ----------------------------------------------------
 * BUILD-DEFINED, DESIGN.md §4.14 (restated by tests/adaptive_ref.py).  A handle in ADAPTIVE mode is tracked and keeps one uint32
 * per shard pixel, frozen_at: 0 = active, else the chunk count K_i at which the pixel froze.  A pass takes the window
 * rayz_hip_progressive_step would take, traces it for the ACTIVE pixels only (every sample keeps its stream, so a chunk sum is
 * the one-shot render's), folds the sums into those pixels' accumulator and moments in chunk order, and freezes every active
 * pixel with chunks_done >= min_chunks and rel2 <= rel_error^2 (the estimate above at K = chunks_done, N = samples_done; a NaN
 * never freezes).  A pixel's value is acc_i * (1 / N_i), N_i = the samples it received: a pixel that never freezes ends as the
 * one-shot pixel bit for bit, a frozen one is the plain handle's preview at chunk K_i bit for bit.  Stopping on a sample
 * variance biases frozen pixels slightly (those whose early chunks happen to agree stop early); min_chunks limits it.
 * rayz_hip_progressive_noise / _noise_rgb evaluate every pixel of an adaptive handle with its own (K_i, N_i) (the summary's
 * samples_done / chunks_done stay the schedule's cursor); rayz_hip_progressive_info's primary_rays counts the samples traced.
 * One device per handle: a shard handle works like any other, several devices are the caller's to combine.  Added in ABI 5
 * (additive). */
#define RAYZ_ADAPTIVE_DEFAULT_MIN_CHUNKS 4u /* a parameter, not contract (provisional) */
typedef struct RayzAdaptiveSummary {
    uint64_t pixels;         /* pixels of the handle's shard */
    uint64_t active;         /* of those, pixels still traced by the next pass */
    uint64_t samples_traced; /* the sum of N_i over the shard's pixels = primary rays so far */
    uint32_t passes;         /* passes that traced something so far */
    uint32_t chunks_done;    /* the schedule cursor: what an active pixel has received */
    uint32_t samples_done;
    uint32_t _pad;
} RayzAdaptiveSummary;
/* Puts `pr` in adaptive mode (and makes it a tracked handle): frozen_at and two active lists, rows_in_shard*width*12 bytes
 * besides the moment state.  RAYZ_ERR_BAD_ARG (checked first): min_chunks < 2 — there is no estimate before the second chunk.
 * RAYZ_ERR_STATE: after the first step.  In adaptive mode rayz_hip_progressive_step and _run_until are RAYZ_ERR_STATE. */
int rayz_hip_progressive_set_adaptive(RayzProgressive* pr, uint32_t min_chunks);
/* One adaptive pass with `min_samples` as rayz_hip_progressive_step takes it.  Blocks: the next pass is sized by the number of
 * pixels this one left active, which `summary_or_null` reports.  THE PREVIEW RULE: a pass writes to `d_preview_or_null` the
 * pixels it traced; a pixel's last write, in the pass it froze in, is its final value, so a buffer passed to every pass holds
 * the whole frame after each.  A pass given another buffer than the previous pass wrote (the first pass, and the pass after
 * one that got NULL: any) writes ALL pixels.  "The same buffer" is the same ADDRESS: the handle does not know whether the memory
 * behind it was freed and allocated again in between, so a caller that replaces its buffer asks for all pixels once, by a pass
 * with NULL before it or a step on the finished run.
 * On a finished run (no pixel active, or the schedule exhausted) the call is RAYZ_OK, traces nothing, moves no cursor, and
 * writes all pixels to the buffer if there is one.  p_or_null as rayz_hip_progressive_noise's (checked first).
 * RAYZ_ERR_STATE: a handle not in adaptive mode. */
int rayz_hip_progressive_adaptive_step(RayzProgressive* pr, const RayzNoiseParams* p_or_null, uint32_t min_samples,
                                       float* d_preview_or_null, RayzAdaptiveSummary* summary_or_null, void* hip_stream);
int rayz_hip_progressive_adaptive_step_f64(RayzProgressive* pr, const RayzNoiseParams* p_or_null, uint32_t min_samples,
                                           double* d_preview_or_null, RayzAdaptiveSummary* summary_or_null, void* hip_stream);
/* Adaptive passes until no pixel is active or the schedule ends; the frame is in `d_preview_or_null`.  Blocks. */
int rayz_hip_progressive_run_adaptive(RayzProgressive* pr, const RayzNoiseParams* p_or_null, uint32_t min_samples_per_pass,
                                      float* d_preview_or_null, RayzAdaptiveSummary* last_summary_or_null, void* hip_stream);
int rayz_hip_progressive_run_adaptive_f64(RayzProgressive* pr, const RayzNoiseParams* p_or_null, uint32_t min_samples_per_pass,
                                          double* d_preview_or_null, RayzAdaptiveSummary* last_summary_or_null, void* hip_stream);
/* N_i, the samples behind every pixel's value (`d_counts`), and frozen_at itself (`d_frozen_at`): rows_in_shard*width uint32
 * each, DEVICE memory, written on `hip_stream` after the handle's last pass.  Block until written.  RAYZ_ERR_STATE: a handle not
 * in adaptive mode; RAYZ_ERR_BAD_ARG: a null buffer. */
int rayz_hip_progressive_sample_counts(RayzProgressive* pr, uint32_t* d_counts, void* hip_stream);
int rayz_hip_progressive_frozen_at(RayzProgressive* pr, uint32_t* d_frozen_at, void* hip_stream);
/* Known answers, as rayz_hip_noise_kat: the fold, the freeze and the compaction of adaptive passes on caller chunk sums (HOST,
 * chunk_sums[(k*n_pixels + i)*3 + ch], chunk_sizes[k] > 0), on the default device; no scene.  Pass p covers the chunks
 * [pass_ends[p-1], pass_ends[p]) (pass_ends strictly increasing, the last <= n_chunks) and is given the compact sums of its
 * active list, as a trace pass would leave them.  `width`: 0 deals the pixels 0, 1, 2, ..; otherwise n_pixels is rows x width
 * and the pixels are dealt as a shard of that shape is (8x8 tiles of whole tile rows where width % 8 == 0, then rows).
 * Outputs (HOST, each optional): frozen_at_out n_pixels; acc_out, q_out, frame_out n_pixels*3 doubles; lists_out
 * (n_passes + 1)*n_pixels — list p, the list pass p traced (list n_passes: what is left), in its first list_sizes_out[p]
 * entries; list_sizes_out n_passes + 1. */
int rayz_hip_adaptive_kat(uint32_t precision, const double* chunk_sums, const uint32_t* chunk_sizes, uint32_t n_pixels,
                          uint32_t n_chunks, const uint32_t* pass_ends, uint32_t n_passes, uint32_t width, uint32_t min_chunks,
                          const RayzNoiseParams* p_or_null, uint32_t* frozen_at_out, double* acc_out, double* q_out,
                          double* frame_out, uint32_t* lists_out, uint32_t* list_sizes_out);

/* ---- sparse renders: a caller's list of pixels, each equal to the frame's own ----------------
 * Traces the `n_pixels` pixels `d_pixels` lists (DEVICE memory) and nothing else.  d_pixels[j] is a LOCAL row-major pixel of
 * `params`' shard, local row * width + column, below rayz_hip_shard_rows(params) * width: the numbering of an adaptive list.
 * Any order; duplicates are allowed.  `params` is the FULL frame's (samples_per_px the total): the chunk schedule, and with it
 * the summation tree, is the frame's, every sample keeps its stream, and entry j receives the three values
 * rayz_hip_render_device gives that pixel, bit for bit.  It writes them at pixel slot d_dest[j] of `d_rgb_out` (DEVICE memory of
 * `dest_pixels` pixel slots, 3 values each) — slot j without `d_dest`, and then dest_pixels must equal n_pixels.  Where two
 * entries name one slot, one of them stays (which is unspecified; the same pixel gives the same bits either way).  A slot no
 * entry names is not written.  `d_var_rgb_out_or_null` (dest_pixels * 3 floats, for both precisions) receives, at the same
 * slots, the per-channel variance of the pixel's mean as rayz_hip_progressive_noise_rgb reports it for a tracked handle that
 * has folded every chunk: +inf for a schedule of one chunk.  max_bounces = 0 writes +0 without tracing.
 * The scene is validated and prepared as for rayz_hip_render_device (AUTO traversal included); the trace runs through the
 * adaptive passes' kernels, so the scan forms and the primary lists do not apply.
 * THE CALL BLOCKS ONCE: every entry is checked on the device first (pixel below the shard's pixel count, slot below dest_pixels)
 * and the host waits for that check's 4-byte count; the trace and the resolve behind it are asynchronous on `hip_stream`.
 * RAYZ_ERR_BAD_ARG, with nothing traced or written: a null camera, params, list or output; a precision that does not match the
 * entry; dest_pixels against the rules above; n_pixels * chunks beyond the work queue's range; any entry out of range.
 * n_pixels = 0 is RAYZ_OK and touches nothing.  Afterwards rayz_hip_scene_sync returns this call's counters: primary_rays =
 * n_pixels * samples_per_px, segments, tests, and kernel_ms between the call's own events (check, trace and resolve). */
int rayz_hip_scene_render_pixels(RayzScene* scene, const RayzCameraDesc* camera, const RayzRenderParams* params,
                                 const uint32_t* d_pixels, uint32_t n_pixels, const uint32_t* d_dest_or_null, uint32_t dest_pixels,
                                 float* d_rgb_out, float* d_var_rgb_out_or_null, void* hip_stream);
int rayz_hip_scene_render_pixels_f64(RayzScene* scene, const RayzCameraDesc* camera, const RayzRenderParams* params,
                                     const uint32_t* d_pixels, uint32_t n_pixels, const uint32_t* d_dest_or_null, uint32_t dest_pixels,
                                     double* d_rgb_out, float* d_var_rgb_out_or_null, void* hip_stream);

/* ---- several GPUs behind ONE call -------------------------------------------------------------------------
 * The reference's caller makes one call, `tracer.render()` (src/rayz.zig:26, src/renderer.zig:72-101).  These
 * entry points give that one call every GPU of the node: the pool is replicated (one scene per device), image
 * rows are dealt to the devices in interleaved tiles of `params->tile_rows` rows (0 = RAYZ_DEFAULT_TILE_ROWS = 8, as everywhere),
 * each device traces its rows on its own stream, and ONE collective — an RCCL gather of the row tiles to
 * devices[0] over xGMI (ncclCommInitAll + ncclGather), or peer copies — reassembles the frame, which is copied
 * to the caller's HOST buffer (height*width*3, row-major RGB).  The image is bit-identical for any device count
 * (the per-(pixel,sample) streams are keyed by global pixel coordinates).  `params->shard_index/shard_count`
 * must be 0: the library shards.  Blocking; driven by the calling thread; one call at a time per handle.
 * A device may be listed once (RAYZ_ERR_BAD_ARG otherwise); OR-ing RAYZ_GATHER_ALLOW_DUPLICATE_DEVICES into a
 * PEER_COPY transport lifts that for TESTS on a one-GPU box (refused with RCCL, which cannot take a device twice).
 * STATUS: with n > 1 DISTINCT devices this path has not yet run on hardware (the development pool has one GPU per
 * box): n = 1 through RCCL and n = 2/3/8 on one device through peer copies are what the GPU suite exercises. */
typedef enum RayzGatherTransport {
    RAYZ_GATHER_RCCL = 0,      /* ncclGather to devices[0] (librccl.so.1 is opened at the first multi-device call) */
    RAYZ_GATHER_PEER_COPY = 1, /* hipMemcpyPeerAsync into devices[0] */
    RAYZ_GATHER_ALLOW_DUPLICATE_DEVICES = 0x100 /* flag bit, peer-copy only: the same ordinal may be listed repeatedly */
} RayzGatherTransport;

typedef struct RayzMulti RayzMulti; /* opaque: one scene per device + communicators + gather buffers */

int rayz_hip_multi_create(const int* devices, int n_devices, const RayzSceneDesc* scene, uint32_t transport,
                          RayzMulti** out);
int rayz_hip_multi_destroy(RayzMulti* multi);
/* n_devices, the transport in use and RCCL's version code (0 with peer copies); any pointer may be NULL */
int rayz_hip_multi_info(const RayzMulti* multi, int* n_devices, uint32_t* transport, int* rccl_version);
/* After a render on the handle: device `index`'s own counters (its rows, its segments, ITS trace-kernel time — load
 * imbalance between row shards shows here), and the frame's timing: gather_ms = on the root's stream, from "the
 * root's rows are traced" to "the frame is assembled" (the transfer + the wait for slower devices + the
 * un-interleave); frame_ms = host wall time of gather + copy-out.  Either pointer of _timing may be NULL. */
int rayz_hip_multi_device_stats(const RayzMulti* multi, int index, RayzRenderStats* stats);
int rayz_hip_multi_timing(const RayzMulti* multi, double* gather_ms, double* frame_ms);
/* `tracer.render()` on all devices of the handle.  stats: counts summed over the devices, kernel_ms = slowest. */
int rayz_hip_multi_render(RayzMulti* multi, const RayzCameraDesc* camera, const RayzRenderParams* params,
                          float* rgb_out, RayzRenderStats* stats_or_null);
int rayz_hip_multi_render_f64(RayzMulti* multi, const RayzCameraDesc* camera, const RayzRenderParams* params,
                              double* rgb_out, RayzRenderStats* stats_or_null);
/* Same frame, but each device applies `Image.writePPM`'s per-pixel transform (src/image.zig:35-38) to its rows
 * BEFORE the gather, so the tiles travel as u8 (4x smaller) and `rgb8_out` (height*width*3 bytes) is what
 * writePPM would print.  f32 precision only. */
int rayz_hip_multi_render_u8(RayzMulti* multi, const RayzCameraDesc* camera, const RayzRenderParams* params,
                             uint8_t* rgb8_out, RayzRenderStats* stats_or_null);
/* One-shot forms: create, render, destroy (RCCL transport).  They pay communicator creation (ncclCommInitAll, tens
 * of milliseconds per device) on EVERY call: a caller that renders more than one frame keeps a RayzMulti. */
int rayz_hip_render_multi(const int* devices, int n_devices, const RayzSceneDesc* scene,
                          const RayzCameraDesc* camera, const RayzRenderParams* params, float* rgb_out,
                          RayzRenderStats* stats_or_null);
int rayz_hip_render_multi_f64(const int* devices, int n_devices, const RayzSceneDesc* scene,
                              const RayzCameraDesc* camera, const RayzRenderParams* params, double* rgb_out,
                              RayzRenderStats* stats_or_null);

/* The step after the path, `Image.writePPM`'s per-pixel transform (src/image.zig:35-38,
 * src/vec.zig:79-93): sqrt-gamma, clamp to [0,1], truncate x*255 to u8.  Device to device,
 * n_pixels*3 floats in, n_pixels*3 bytes out. */
int rayz_hip_tonemap_u8(const float* d_rgb, uint8_t* d_rgb8, size_t n_pixels, void* hip_stream); /* default device */

/* ---- known answers ---------------------------------------------------------------------------------------------
 * Evaluates the trace kernels' OWN device functions (the same inlined code the kernels run) on caller inputs, one
 * GPU thread per record, so that the reference's test vectors and a CPU restatement can be held against the
 * device code directly.  Covered: everything a path is assembled from, the BVH kernels' leaf reject test
 * (leaf_reject_test, shared with the walk) and the flat list's packed-FMA form of it (ScanGroup::discs, two spheres
 * per v_pk_fma_f32: RAYZ_KAT_SCAN_DISCS; in the scan loop its sphere operands come from scalar registers, here from
 * vector ones — the same arithmetic) included.  Vectors: src/material.zig:213-223 (refract), src/renderer.zig:129-149 (get ray),
 * src/hit.zig:247-279 (bbox hit); tests/test_kat_gpu.py.  Host buffers: `in` = n records of RAYZ_KAT_IN_STRIDE
 * doubles, `out` = n records of RAYZ_KAT_OUT_STRIDE doubles (unused slots 0).  Values are narrowed to `precision`
 * as a scene is when it crosses the ABI.  Random draws, where an op makes any, come from the record's list u[]
 * (0.5 beyond its end) in the order the path would make them.  Default device. */
typedef enum RayzKatOp {
    RAYZ_KAT_REFRACT = 0,     /* in: unit_dir[0..2] normal[3..5] eta[6]            out: dir[0..2]       src/material.zig:189-194 */
    RAYZ_KAT_REFLECTANCE = 1, /* in: cos[0] ri[1]                                  out: r[0]            src/material.zig:179-183 */
    RAYZ_KAT_GET_RAY = 2,     /* in: look_from px_du px_dv px_origin defocus_u defocus_v [0..17] defocus[18] px[19] py[20]
                                     n_u[21] (an integer in [0, 26], or -1; RAYZ_ERR_BAD_ARG otherwise) u[22..];
                                     n_u = -1 is getRay(px, py, null) — no jitter, lens centre, time 0: the call of the reference's own
                                     "get ray" test, src/renderer.zig:129-149; n_u = 0 draws 0.5 everywhere (the kernels always draw)
                                 out: origin[0..2] dir[3..5] time[6] draws[7]                           src/camera.zig:59-90 */
    RAYZ_KAT_BOX_HIT = 3,     /* in: low[0..2] high[3..5] origin[6..8] dir[9..11] tmin[12] tmax[13] format[26] (the node record
                                     the box is tested in: 0 = 16-bit plane indices, non-zero = f32 planes)
                                 out: hit[0] t_entry[1]                                                 src/hit.zig:70-98 */
    RAYZ_KAT_SPHERE_HIT = 4,  /* in: center[0..2] velocity[3..5] radius[6] origin[7..9] dir[10..12] time[13] tmin[14] tmax[15]
                                 out: hit[0] t[1] point[2..4] normal[5..7] front_face[8] passed_filter[9]
                                                                                        src/geom.zig:38-66, src/hit.zig:25-41 */
    RAYZ_KAT_SCATTER = 5,     /* in: kind[0] method[1] param[2] ray origin[3..5] dir[6..8] hit point[9..11] normal[12..14]
                                     front_face[15] n_u[16] (an integer in [0, 31]) u[17..]
                                 out: scattered[0] dir[1..3] draws[4]                                   src/material.zig:73-160 */
    RAYZ_KAT_CHECKER = 6,     /* in: point[0..2] scale[3]                          out: parity[0]       src/material.zig:32-36 */
    RAYZ_KAT_BACKGROUND = 7,  /* in: dir[0..2]                                     out: colour[0..2]    src/renderer.zig:124-125 */
    RAYZ_KAT_TRIANGLE_HIT = 8,/* in: v0[0..2] v1[3..5] v2[6..8] origin[9..11] dir[12..14] tmin[15] tmax[16]
                                 out: hit[0] t[1] passed_filter[2]                 build-defined */
    RAYZ_KAT_SCAN_DISCS = 9,  /* one 4-sphere block of the flat list's scan streams, as the SCAN LOOP evaluates it (packed FMAs,
                                 two spheres per instruction; the values are f32 for both precisions):
                                 in: cx[0..3] cy[4..7] cz[8..11] radius[12..15] (padded and squared by the library as the scene
                                     upload does) vy[16..19] origin[20..22] dir[23..25] time[26] class[27]: 0 static, 1 y-moving
                                     (the loose forms, ScanGroup<float, 0 / 1>), 2 static, 3 y-moving PLANE RUN (the run forms,
                                     ScanGroup<float, 3 / 4>: the run's height is cy[4], K2 = fm(cy, e2y, k2) as the run loop
                                     computes it; the four cy must be one f32 value, bit for bit); any other class, or a plane-run
                                     record whose cy differ in f32, is RAYZ_ERR_BAD_ARG; want_r2[32] (0 or 1, RAYZ_ERR_BAD_ARG
                                     otherwise): 1 returns the padded r2 below, for any class
                                 out: r2 - p1^2 - p2^2 per sphere [0..3] (>= 0: candidate; the plane form for classes 2 / 3), the
                                      same value from the general-velocity form the BVH leaves use [4..7], the padded r2 (f32) the
                                      library used [8..11] if want_r2, else 0              src/geom.zig:40-50, DESIGN.md 4.3 */
    RAYZ_KAT_BUCKET_DISCS = 10, /* one 4-sphere block of a SPEED BUCKET of a y-moving plane run, as the scan loop evaluates it
                                 (ScanGroup<float, 5>: the static plane form, the bucket's speed folded into K2):
                                 in: cx[0..3] cy[4] (the run's height) cz[8..11] radius[12..15] vy[16..19] origin[20..22]
                                     dir[23..25] time[26] v0[27] (the bucket's speed; finite, RAYZ_ERR_BAD_ARG otherwise)
                                 out: r2b - p1^2 - p2^2 per sphere [0..3], K2 = fm(v0, time * e2y, fm(cy, e2y, k2)) [4], the
                                      padded r2b (f32) of radius + |vy - v0| the library used [8..11]      DESIGN.md 4.3 */
    RAYZ_KAT_SCAN_DISCS_XY = 11, /* RAYZ_KAT_SCAN_DISCS' record (same fields, same checks) through the reject test's XY basis
                                 (RAYZ_SCAN_FORM_XY: e1 in the xy-plane; a plane run folds its height into K1 and K2 and tests
                                 a sphere pair in 5 packed FMAs):
                                 out: r2 - p1^2 - p2^2 per sphere [0..3], the k1 and k2 the block was tested with [4] [5] (a
                                      plane run's K1 = fm(cy, e1y, k1), K2 = fm(cy, e2y, k2)), e1x [6], e1y [7], the padded r2
                                      [8..11] if want_r2, else 0                                            DESIGN.md 4.3 */
    RAYZ_KAT_BUCKET_DISCS_XY = 12, /* RAYZ_KAT_BUCKET_DISCS' record through the XY basis:
                                 out: r2b - p1^2 - p2^2 per sphere [0..3], K1 = fm(v0, time * e1y, fm(cy, e1y, k1)) [4],
                                      K2 = fm(v0, time * e2y, fm(cy, e2y, k2)) [5], e1x [6], e1y [7], the padded r2b [8..11] */
    RAYZ_KAT_SET_DISCS = 13     /* one 8-sphere block of a ONE-RADIUS SET of a static plane run or a speed bucket, as the set loop
                                 evaluates it (RAYZ_SCAN_FORM_ONE_RADIUS: the XY basis, cx and cz from the block, one padded R2):
                                 in: cx[0..7] cz[8..15] cy[16] (the run's height) v0[17] (the bucket's speed; finite) Rp[18] (the
                                     set's one radius, >= every member's |radius| + |vy - v0|; finite, >= 0) movy[19] (0: a static
                                     run's set, v0 and vy unused; 1: a bucket's) origin[20..22] dir[23..25] time[26] vy[28..35]
                                     (RAYZ_ERR_BAD_ARG for a bad v0, Rp or movy)
                                 out: R2 - p1^2 - p2^2 per sphere [0..7], the K1 and K2 the block was tested with [8] [9], the
                                      padded R2 (f32) the library used: the largest over the eight members [10]    DESIGN.md 4.3 */
} RayzKatOp;
#define RAYZ_KAT_IN_STRIDE 48
#define RAYZ_KAT_OUT_STRIDE 12
int rayz_hip_kat(uint32_t op, uint32_t precision, const double* in, uint32_t n_records, double* out);

/* ---- ray queries: "what does this ray hit?" ------------------------------------------------------------------
 * The reference's other interface, `BVH.findHit(hittables, ray, tmin, tmax) -> ?Hit` (src/hit.zig:181-217, the sphere test
 * src/geom.zig:33-66, the record `Hit.init` src/hit.zig:25-41), on a batch of rays held in DEVICE memory, against a scene created
 * with rayz_hip_scene_create: the render's own scan or BVH walk, reject test, f64 narrow phase and tie rule (nearest, ties to the
 * larger hittable index), with the root accepted in [tmin, tmax] — both ends inclusive, as in the reference.
 * Hittables are numbered spheres first, then triangles.  Added in ABI 5 (additive: no existing symbol changed).
 * Queries leave rayz_hip_scene_sync's counters alone and change nothing of a progressive handle stepped between them; a scene
 * still has ONE render or query in flight (a query on another stream first waits for the scene's last launch). */
typedef enum RayzQueryKind {
    RAYZ_QUERY_NEAREST = 0, /* the `findHit` result: hittable, t, point, normal, front_face, material, albedo */
    RAYZ_QUERY_ANY = 1      /* occlusion: is there a root in [tmin, tmax]?  A lane's BVH walk ends at the first one */
} RayzQueryKind;

typedef struct RayzQueryParams {
    uint32_t n_rays;    /* 0: a no-op that returns RAYZ_OK */
    uint32_t kind;      /* RayzQueryKind */
    uint32_t precision; /* RayzPrecision: the type of the rays and of the R outputs.  F32 holds rays in f32 and decides candidates in
                           f64 on the pool's spheres; F64 is f64 throughout (as renders) */
    uint32_t traversal; /* RayzTraversal.  AUTO uses RAYZ_AUTO_BVH_MIN, a crossover measured for PATH TRACING, not for queries */
    double tmin;        /* the same for every ray (a NaN is RAYZ_ERR_BAD_ARG) */
} RayzQueryParams;

/* Where the results go: DEVICE memory, each pointer optional (NULL = not written).  R = float or double by the precision.
 * NEAREST writes every field it is given; ANY writes `hit` only.  On a miss: index and material -1, t +inf, point, normal and
 * albedo 0, front_face 0. */
typedef struct RayzQueryOutputs {
    int32_t* index;     /* n: hittable index, or -1 */
    void* t;            /* n R */
    void* point;        /* 3n R: o + t·d as shade computes it */
    void* normal;       /* 3n R: unit outward normal, flipped to face the ray (Hit.init) */
    uint8_t* front_face;/* n: 1 if the ray hit the outside */
    int32_t* material;  /* n: MaterialHandle.idx, or -1 */
    void* albedo;       /* 3n R: texture_value at the point; (1, 1, 1) for a dielectric */
    uint8_t* hit;       /* n: 1 if a root lies in [tmin, tmax] (either kind) */
} RayzQueryOutputs;

/* A batch of rays: `d_rays` is DEVICE memory, n_rays x 8 values of the precision, {ox, oy, oz, time, dx, dy, dz, tmax} per ray.
 * Refused with RAYZ_ERR_BAD_ARG: a NaN or infinite origin, direction or time, an origin component beyond RAYZ_QUERY_MAX_ORIGIN,
 * a zero direction, a direction whose largest |component| lies outside [RAYZ_QUERY_MIN_DIR, RAYZ_QUERY_MAX_DIR], a NaN tmax, a time outside [0, 1] (the BVH's moving-sphere boxes enclose the centre over [0, 1] only,
 * Sphere.boundingBox).  tmax < tmin is allowed: a miss.
 * BLOCKING PART: a small reduction kernel over the batch finds max |origin|, the time range and the refusals, and the host waits for
 * those few values (the scan's reject radii and the BVH's f32 boxes are padded for a bound on every ray origin, DESIGN.md §4.3 /
 * §4.8: the scene's buffers are rebuilt if they were padded for less).  The query itself then runs asynchronously on
 * `hip_stream` (NULL: the library's stream); rayz_hip_query_sync waits for it.  `d_rays` and the outputs must stay allocated
 * until then.
 * PADDING IS NEVER SHRUNK: a batch whose origins lie farther out than the scene's and the cameras' own bound widens the scene's
 * reject radii and boxes for good (for twice that bound), so later renders and queries on the scene test more candidates and
 * boxes — the same images, more work.  A caller that queries from far away and then renders again keeps a second scene. */
#define RAYZ_QUERY_MAX_ORIGIN 1e9 /* largest |origin component| a query accepts: the padding stays finite in f32 */
/* The accepted scale of a direction, 2^-32 <= max_k |d_k| <= 2^32.  `findHit` does not depend on the scale of d (d·2^k with
 * tmin, tmax·2^-k is the same hit at t·2^-k), but the arithmetic does: beyond about 2^58 (F32: unit(d)'s d·d and the triangle
 * test's det² overflow f32) and below about 2^-56 (the BVH's 1/d_k is capped at 2^64; F32: d·d underflows), and for F64 beyond
 * the ±2^100 hold on d_k in front of the f32 box test, true hits are lost without an error.  The range keeps a factor of at least
 * 2^16 to the first lost hit of every piece (measured on the CPU restatement: tests/test_query_exact_cpu.py).  This refusal, in
 * ABI 5 as the others, rejects only inputs that gave wrong answers before. */
#define RAYZ_QUERY_MIN_DIR 2.3283064365386962890625e-10 /* 2^-32 */
#define RAYZ_QUERY_MAX_DIR 4294967296.0                 /* 2^32 */
int rayz_hip_scene_query(RayzScene* scene, const RayzQueryParams* query, const void* d_rays, const RayzQueryOutputs* outputs,
                         void* hip_stream);
/* The camera form: one ray per pixel of the shard `params` describes, camera_ray_no_rng — `getRay(px, py, null)`: the pixel's
 * centre, the lens centre, time 0, tmax +inf — a G-buffer.  Output entry = local row · width + column (rows_in_shard x width),
 * as renders store pixels.  Reads width, height, shard_index, shard_count, tile_rows, precision, traversal and tmin of
 * `params`; ignores samples_per_px, max_bounces, seed and chunk_spp.  Kind NEAREST.  Asynchronous, nothing blocks. */
int rayz_hip_scene_query_camera(RayzScene* scene, const RayzCameraDesc* camera, const RayzRenderParams* params,
                                const RayzQueryOutputs* outputs, void* hip_stream);
/* Waits for the scene's last query and returns its counters: primary_rays = segments = rays, node_tests and sphere_tests as
 * renders count them (flat list: rays x hittables), kernel_ms = the query kernel's HIP-event time. */
int rayz_hip_query_sync(RayzScene* scene, RayzRenderStats* stats_or_null);

/* ---- specular-chain G-buffers: guides seen through mirrors and glass -------------------------------
 * BUILD-DEFINED.  rayz_hip_scene_query_camera with the ray FOLLOWED through mirror-like metals and dielectrics: per pixel,
 * segment 0 is the camera query's ray; while the nearest hit of a segment is a dielectric, or a metal whose fuzz is at most
 * `max_fuzz`, and fewer than `max_depth` hits have been followed, the next segment starts at the hit point (time 0, tmax +inf,
 * the call's tmin) along the direction `Material.scatter` gives with the metal's fuzz taken as 0 and every uniform draw 1.0:
 * unit(reflect(d, n)) off a metal; through a dielectric the refraction unless eta·sin > 1 (then the reflection), never the
 * Fresnel reflection.  A metal that absorbs the ray (its reflection points into the surface) ends the chain on that hit.
 * `outputs` receives the record of the LAST segment exactly as a NEAREST query of that segment's ray writes it — so point,
 * normal and index are those of the first non-specular surface along the path, or a miss — except `albedo`, which is that
 * record's albedo multiplied per channel by the albedos of the followed hits (1, 1, 1 for glass).
 * Reads the same fields of `params` as rayz_hip_scene_query_camera, deals pixels and shards the same way, is asynchronous the
 * same way (rayz_hip_query_sync waits for it: primary_rays = pixels, segments = the sum of depth + 1 over them), and counts as
 * the scene's one render or query in flight.  max_depth = 0 is rayz_hip_scene_query_camera bit for bit.
 * RAYZ_ERR_BAD_ARG before any HIP call: as rayz_hip_scene_query_camera, and max_depth > RAYZ_CHAIN_MAX_DEPTH, a max_fuzz that
 * is NaN or negative.  `chain` NULL: the defaults.  Added in ABI 5 (additive: no existing symbol or struct changed).
 * The record is NOT a first-hit record: temporal reprojection (rayz_hip_temporal_*) needs the first-hit point, so a caller that
 * uses both fills two G-buffers per frame. */
#define RAYZ_CHAIN_MAX_DEPTH 16u
#define RAYZ_CHAIN_DEFAULT_DEPTH 4u      /* a hollow glass ball is four interfaces; a parameter, provisional */
#define RAYZ_CHAIN_DEFAULT_MAX_FUZZ 0.25 /* a parameter, provisional */
typedef struct RayzChainParams {
    uint32_t max_depth; /* hits followed at most, 0..RAYZ_CHAIN_MAX_DEPTH */
    uint32_t _pad;
    double max_fuzz;    /* a metal whose fuzz (narrowed to the precision) is greater is not followed */
} RayzChainParams;
typedef struct RayzChainOutputs { /* DEVICE memory, each optional; entries as RayzQueryOutputs' */
    uint32_t* key;         /* n: the chain key: 0, then key <- key x 0x9E3779B1 + (index + 1) in uint32 arithmetic for every followed
                              hit; 0 for a pixel whose first hit was not followed */
    uint8_t* depth;        /* n: number of hits followed */
    int32_t* first_index;  /* n: what rayz_hip_scene_query_camera's `index` holds */
} RayzChainOutputs;
int rayz_hip_scene_query_camera_chain(RayzScene* scene, const RayzCameraDesc* camera, const RayzRenderParams* params,
                                      const RayzChainParams* chain_or_null, const RayzQueryOutputs* outputs,
                                      const RayzChainOutputs* chain_outputs_or_null, void* hip_stream);

/* ---- sampled G-buffers: guide means over the render's own camera rays --------------------------------
 * BUILD-DEFINED.  rayz_hip_scene_query_camera traces the pixel's centre through the lens centre at time 0; the frame it guides
 * is made of samples jittered over the pixel, the lens disk and the shutter.  This call traces those: for every pixel (px, py)
 * (global coordinates) of the shard `params` describes, dealt and stored as rayz_hip_scene_query_camera does it, and with
 * spp = params->samples_per_px, samples s = 0 .. n-1:
 *   ray     a Pcg32 seeded with seed_path(params->seed, (py·width + px)·spp + s), then camera_ray (jitter
 *           x, jitter y, the lens tries if the camera has a defocus disk, time); tmin = params->tmin, tmax = +inf.  It IS the
 *           camera segment of the render's path s of that pixel, bit for bit.
 *   record  the NEAREST findHit record of that ray as a query writes it (by params->traversal, AUTO as for queries, in
 *           params->precision R): hit or miss, t, the normal facing the ray, the albedo (texture_value at the point; (1, 1, 1)
 *           for a dielectric).
 *   sums    in R, from +0, one add (one rounding) per sample in sample order: hits (uint32) counts the hit samples;
 *           A_k += albedo_k on a hit and A_k += 1 on a miss; N_k += normal_k and T += t on a hit only.
 * Outputs (RayzSampledOutputs: DEVICE memory, each optional, entry = local row · width + column): albedo = A_k / (R)n; normal =
 * N_k / (R)hits, (0, 0, 0) when hits = 0 — NOT normalised: its length says how far the samples' normals agree; t = T / (R)hits,
 * +inf when hits = 0; hits.  Every divide is correctly rounded; there is no other arithmetic.  So n = 1 writes the one ray's
 * NEAREST record (0 + x, x / 1: x but for the sign of a zero), the result does not depend on traversal, node format, shard count
 * or launch shape, and the guides of a frame rendered with the same `params` are means over that frame's own camera segments.
 * `sampled` NULL or samples = 0: n = spp.  RAYZ_ERR_BAD_ARG before any HIP call: everything
 * rayz_hip_scene_query_camera_chain refuses, spp = 0, samples > spp (the ids would run into the next pixel's paths), `outputs`
 * NULL.  Reads width, height, shard_index, shard_count, tile_rows, precision, traversal, tmin, samples_per_px and seed of
 * `params` and ignores the rest.  Asynchronous as the camera query; counts as the scene's one render or query in flight;
 * rayz_hip_query_sync waits for it and reports primary_rays = segments = pixels · n, node and sphere tests as for queries.  It
 * leaves rayz_hip_scene_sync's counters and every progressive handle alone and changes no frame any other entry point produces.
 * For n > 1 the scene keeps a workspace of 8 R per pixel of the largest shard asked for.  Added in ABI 5 (additive: no existing
 * symbol or struct changed). */
typedef struct RayzSampledParams {
    uint32_t samples; /* n: 1 .. params->samples_per_px; 0 = samples_per_px */
    uint32_t _pad;
} RayzSampledParams;
typedef struct RayzSampledOutputs { /* DEVICE memory, each optional; R by the precision */
    void* albedo;   /* 3n R: mean albedo, a miss counting as (1, 1, 1) */
    void* normal;   /* 3n R: mean over the hit samples of the normal facing the ray; not normalised; 0 when hits = 0 */
    void* t;        /* n R: mean t over the hit samples; +inf when hits = 0 */
    uint32_t* hits; /* n: the hit samples */
} RayzSampledOutputs;
int rayz_hip_scene_query_camera_sampled(RayzScene* scene, const RayzCameraDesc* camera, const RayzRenderParams* params,
                                        const RayzSampledParams* sampled_or_null, const RayzSampledOutputs* outputs,
                                        void* hip_stream);

/* ---- denoising: a G-buffer-guided à-trous filter for low-spp frames -------------------------------------------------
 * BUILD-DEFINED (the reference has no denoiser): an edge-avoiding à-trous wavelet filter (Dammertz et al. 2010) on a WHOLE f32
 * frame in DEVICE memory, guided by the G-buffer a rayz_hip_scene_query_camera call of F32 precision filled for the same camera
 * and frame size.  The arithmetic is a contract, DESIGN.md §4.11 (+ - x, explicit FMAs, correctly rounded divides, comparisons;
 * no transcendental), restated bit for bit on the CPU by tests/denoise_mirror.cpp.  Added in ABI 5 (additive: no existing symbol
 * changed); it changes no image any other entry point produces.
 * Limits of this version: whole frames only (rows of a shard are not image neighbours: gather first); f32 only.  With the
 * G-buffer of rayz_hip_scene_query_camera the guides are FIRST-HIT guides, so what a metallic or dielectric surface reflects or
 * refracts is filtered as if it were painted on it; the G-buffer of rayz_hip_scene_query_camera_chain with its keys
 * (rayz_hip_denoiser_set_keys) guides the filter by what is SEEN in such a surface instead. */
typedef struct RayzDenoiser RayzDenoiser; /* opaque: packed guides + two colour buffers for one frame size on one device */

#define RAYZ_DENOISE_ALBEDO 0x1u      /* demodulate: filter c / max(albedo, 2^-8) and multiply it back in (needs gbuffer->albedo) */
#define RAYZ_DENOISE_DEFAULT_LEVELS 5u
#define RAYZ_DENOISE_DEFAULT_NORMAL_POWER_LOG2 6u
#define RAYZ_DENOISE_DEFAULT_SIGMA_COLOR 0.5  /* the sigmas: picked on the CPU restatement; parameters, not contract */
#define RAYZ_DENOISE_DEFAULT_SIGMA_PLANE 0.25
#define RAYZ_DENOISE_MAX_PIXELS 1073741824u /* 2^30: the largest width*height a handle accepts (RAYZ_ERR_BAD_ARG beyond) */

typedef struct RayzDenoiseParams {
    uint32_t levels;            /* 1..8 levels of stride 1, 2, 4, ..; 0 = RAYZ_DENOISE_DEFAULT_LEVELS */
    uint32_t normal_power_log2; /* the normal weight max(0, n_p.n_q) is squared this many times, 0..16 (taken as given: 0 = not squared) */
    uint32_t flags;             /* RAYZ_DENOISE_ALBEDO or 0 */
    uint32_t _pad;
    double sigma_color;         /* > 0; +inf switches the colour term off exactly.  Used as f32; its f32 square must be > 0 */
    double sigma_plane;         /* > 0: the sine of the angle out of the centre pixel's tangent plane at which a tap's weight reaches 0 */
} RayzDenoiseParams;

/* device < 0: the default device (RAYZ_ERR_NO_DEVICE before rayz_hip_init); otherwise creates that device's context if needed.
 * RAYZ_ERR_BAD_ARG: a zero size, or width*height > RAYZ_DENOISE_MAX_PIXELS. */
int rayz_hip_denoiser_create(int device, uint32_t width, uint32_t height, RayzDenoiser** out);
/* d_rgb_in, d_rgb_out: DEVICE memory, height*width*3 floats, packed RGB as renders write it; d_rgb_out == d_rgb_in is allowed.
 * `gbuffer`: index, normal and point are required, albedo unless RAYZ_DENOISE_ALBEDO is off; the other fields are ignored.
 * params == NULL: all defaults.  Asynchronous on `hip_stream` (NULL: the library's stream of the handle's device); the inputs
 * must stay allocated until the run has finished.  One run in flight per handle: a run first makes its stream wait, on the
 * device, for the handle's previous run (through an event of the handle's own, so the previous run's stream may have been
 * destroyed by then; _destroy waits the same way).
 * RAYZ_ERR_BAD_ARG (checked before the handle, without touching a device): levels > 8, normal_power_log2 > 16, a sigma that is
 * not positive (NaN included), unknown flag bits, a missing required pointer.  RAYZ_ERR_STATE: a bad handle. */
int rayz_hip_denoiser_run(RayzDenoiser* dn, const RayzDenoiseParams* params, const float* d_rgb_in,
                          const RayzQueryOutputs* gbuffer, float* d_rgb_out, void* hip_stream);
/* ---- variance-guided denoising ----
 * The spatial stage of SVGF (Schied et al. 2017) on the same handle and guides: the colour distance of a tap is measured in units
 * of the centre pixel's own variance, so a pixel that has converged keeps its detail and one that has not is smoothed.
 * `d_var_rgb`: DEVICE memory, height*width*3 floats, the variance of each channel of d_rgb_in's pixel means
 * (rayz_hip_progressive_noise_rgb writes exactly this).  It is demodulated with the colour, summed over the channels, smoothed
 * 3x3 per level and filtered along with the colour (weights squared), so every level sees the variance its input has.  A NaN,
 * +inf (no estimate yet) or huge variance is taken as 2^32: that pixel trusts the guides only.  A tap's colour weight is
 * 1 / (1 + |de|^2 / (sigma_color^2 x (variance + var_floor))): `sigma_color` is in STANDARD DEVIATIONS here, and `var_floor`
 * keeps a pixel whose estimate is 0 (a black or a constant pixel) from refusing every neighbour.  The arithmetic is a contract
 * (§4.13, the rules of §4.11), restated bit for bit by tests/denoise_guided_mirror.cpp.  Added in ABI 5 (additive). */
#define RAYZ_DENOISE_GUIDED_DEFAULT_LEVELS 5u
#define RAYZ_DENOISE_GUIDED_DEFAULT_SIGMA_COLOR 2.0 /* these three: DESIGN.md §6 says what they rest on; parameters, not contract */
#define RAYZ_DENOISE_GUIDED_DEFAULT_VAR_FLOOR 1e-4

typedef struct RayzDenoiseGuidedParams {
    uint32_t levels;            /* as RayzDenoiseParams; 0 = RAYZ_DENOISE_GUIDED_DEFAULT_LEVELS */
    uint32_t normal_power_log2; /* as RayzDenoiseParams */
    uint32_t flags;             /* RAYZ_DENOISE_ALBEDO or 0 */
    uint32_t _pad;
    double sigma_color;         /* > 0, in standard deviations; +inf switches the colour term off exactly.  Used as f32; its f32 square must be > 0 */
    double sigma_plane;         /* as RayzDenoiseParams */
    double var_floor;           /* > 0, added to every pixel's variance.  Used as f32; f32(sigma_color)^2 x f32(var_floor) must be > 0 in f32 */
} RayzDenoiseGuidedParams;

/* As rayz_hip_denoiser_run (buffers, stream, the one run in flight per handle — of either mode —, timing, in place allowed), plus
 * `d_var_rgb` (required) and `d_var_out_or_null`: DEVICE memory, height*width floats, the variance left in the DEMODULATED colour
 * after the last level, channels summed (multiply by the squared modulation for a radiance variance).  params == NULL: all defaults.
 * RAYZ_ERR_BAD_ARG as rayz_hip_denoiser_run, and: a var_floor that is not positive (NaN included) or whose f32 product with
 * sigma_color^2 is not; d_var_rgb == NULL. */
int rayz_hip_denoiser_run_guided(RayzDenoiser* dn, const RayzDenoiseGuidedParams* params, const float* d_rgb_in,
                                 const float* d_var_rgb, const RayzQueryOutputs* gbuffer, float* d_rgb_out,
                                 float* d_var_out_or_null, void* hip_stream);
/* rayz_hip_denoiser_run_guided with a TAP: while it runs it also writes to `d_tap_rgb` (DEVICE memory, height*width*3 floats) the
 * re-modulated colour after `tap_level` levels — bit for bit what rayz_hip_denoiser_run_guided with levels = tap_level writes to its
 * d_rgb_out.  d_rgb_out and d_var_out are what the untapped run writes.  1 <= tap_level <= levels; tap_level = 1 is the image SVGF
 * feeds back into its colour history (rayz_hip_temporal_feedback).  The tap costs one more 12-byte store per pixel in the tapped
 * level (and that level's read of the modulation record, unless it is the last).  RAYZ_ERR_BAD_ARG (before the handle) as
 * rayz_hip_denoiser_run_guided, and: tap_level 0 or above the resolved `levels`; d_tap_rgb NULL, or equal to d_rgb_in or d_rgb_out. */
int rayz_hip_denoiser_run_guided_tap(RayzDenoiser* dn, const RayzDenoiseGuidedParams* params, const float* d_rgb_in,
                                     const float* d_var_rgb, const RayzQueryOutputs* gbuffer, float* d_rgb_out,
                                     float* d_var_out_or_null, uint32_t tap_level, float* d_tap_rgb, void* hip_stream);
/* Waits for the handle's last run and returns its HIP-event times: *levels_or_null = L, the levels it ran; ms_or_null[0] = the
 * pack pass, ms_or_null[1 + l] = level l, for as many of the L + 1 entries as `capacity` holds.  RAYZ_ERR_STATE before any run. */
/* Surface keys: every LATER run on the handle, of either mode, with or without a tap, reads height*width keys
 * from `d_keys_or_null` (DEVICE memory) in its pack pass, and a tap whose key differs from the centre pixel's, compared as a
 * 32-bit integer, is skipped exactly as a tap outside the frame is — before anything else, background taps and the guided
 * mode's 3x3 variance prefilter included.  rayz_hip_scene_query_camera_chain's `key` keeps "the ground" and "the ground seen in
 * the ball" apart at the ball's silhouette.  NULL, the initial state, turns keys off: every image is what it was without this
 * entry, bit for bit (so is one with all keys equal).  The buffer must stay allocated while runs use it.  Changes nothing on a
 * device.  RAYZ_ERR_STATE: a bad handle. */
int rayz_hip_denoiser_set_keys(RayzDenoiser* dn, const uint32_t* d_keys_or_null);
int rayz_hip_denoiser_timing(RayzDenoiser* dn, uint32_t* levels_or_null, float* ms_or_null, uint32_t capacity);
int rayz_hip_denoiser_destroy(RayzDenoiser* dn);

/* ---- guided upscaling: a low-resolution frame under a full-size G-buffer ---------------------------
 * BUILD-DEFINED.  A frame traced at 1/f of the resolution in each direction (f = 2, 3 or 4; the camera of
 * render.lowres_camera: every low-resolution pixel sits at the centre of its f x f block of full pixels) is rebuilt at full size:
 * every full pixel takes the 2x2 low-resolution pixels around it, weighs each by its bilinear weight times the GUIDE weight of
 * the denoiser's tap — the full pixel's normal and point from `gbuffer_hi` against the low-resolution pixel's from `gbuffer_lo`;
 * background never mixes with a hit —, interpolates the colour DEMODULATED by the low-resolution albedo and multiplies its own
 * full-size albedo back in, so texture detail comes back at full resolution and no colour crosses a silhouette.  A pixel whose
 * 2x2 footprint holds nothing it may mix with (stage 1) tries the 4x4 footprint with the guide weight alone; failing that
 * (stage 2) it takes the nearest low-resolution pixel's raw colour.  The arithmetic is a contract (§4.20, the rules of §4.11),
 * restated bit for bit by tests/upscale_mirror.cpp.  Added in ABI 5 (additive: no existing symbol or struct changed).
 * Limits of this version: whole frames, f32 only; the full size is an exact multiple of the factor; surface keys are not used (a
 * chain G-buffer is accepted as plain guides). */
typedef struct RayzUpscaler RayzUpscaler; /* opaque: the packed low-resolution records (80 bytes per low-resolution pixel) */

#define RAYZ_UPSCALE_FORM_AUTO 0u   /* the build's choice */
#define RAYZ_UPSCALE_FORM_DIRECT 1u /* the 2x2 footprint read through L1 / L2: the only form this version has */

typedef struct RayzUpscaleParams {
    uint32_t factor;            /* 2..4, and the handle's */
    uint32_t normal_power_log2; /* as RayzDenoiseParams */
    uint32_t flags;             /* RAYZ_DENOISE_ALBEDO or 0 */
    uint32_t form;              /* RAYZ_UPSCALE_FORM_*: how the taps are fetched, never what they give */
    double sigma_plane;         /* as RayzDenoiseParams */
} RayzUpscaleParams;

/* `width` x `height` is the FULL frame.  device as rayz_hip_denoiser_create.  RAYZ_ERR_BAD_ARG (before any HIP call): a factor
 * outside 2..4, a zero size or one that is no multiple of the factor, width*height > RAYZ_DENOISE_MAX_PIXELS. */
int rayz_hip_upscaler_create(int device, uint32_t width, uint32_t height, uint32_t factor, RayzUpscaler** out);
/* With (h, w) = (height, width) / factor.  d_rgb_lo: DEVICE memory, h*w*3 floats, the low-resolution frame; d_var_rgb_lo_or_null:
 * h*w*3 floats, the variance of each channel of its pixel means (rayz_hip_progressive_noise_rgb, or the variance a
 * rayz_hip_temporal_step writes).  `gbuffer_lo`, `gbuffer_hi`: index, normal and
 * point are required, albedo with RAYZ_DENOISE_ALBEDO; F32 camera queries at h x w and at height x width.  d_rgb_out:
 * height*width*3 floats.  d_var_rgb_out_or_null: height*width*3 floats, each full pixel's MARGINAL variance per channel
 * (neighbouring full pixels share taps: their errors are correlated, §4.20); 2^32 where stage 2 had no estimate; needs
 * d_var_rgb_lo.  d_stage_out_or_null: height*width bytes, the stage (0, 1 or 2) that produced each pixel.  No output may overlap
 * an input or another output.  `params` is required (the factor has no default).  Asynchronous on `hip_stream`, one run in flight
 * per handle, as rayz_hip_denoiser_run.
 * RAYZ_ERR_BAD_ARG (checked before the handle, without touching a device): params NULL, a factor outside 2..4,
 * normal_power_log2 > 16, unknown flag bits, a form this build does not have, a sigma_plane that is not positive (NaN included),
 * a missing required pointer, a G-buffer without index, normal or point, RAYZ_DENOISE_ALBEDO without the albedo of both
 * G-buffers, a variance output without the variance input, an output equal to an input or another output.  RAYZ_ERR_STATE: a
 * bad handle.  RAYZ_ERR_BAD_ARG behind it: a factor that is not the handle's, an output overlapping an input. */
int rayz_hip_upscaler_run(RayzUpscaler* up, const RayzUpscaleParams* params, const float* d_rgb_lo,
                          const float* d_var_rgb_lo_or_null, const RayzQueryOutputs* gbuffer_lo,
                          const RayzQueryOutputs* gbuffer_hi, float* d_rgb_out, float* d_var_rgb_out_or_null,
                          uint8_t* d_stage_out_or_null, void* hip_stream);
/* The same run for a LATTICE frame (DESIGN.md 4.20 "Lattice samples", 4.21): low-resolution pixel (i, j) IS full pixel
 * (factor*i + phase_x, factor*j + phase_y) — the frame render.lattice_pixels lists and rayz_hip_scene_render_pixels traces, with
 * `gbuffer_lo` the same pixels of `gbuffer_hi` — not the mean of a block.  The position of a full pixel among the samples
 * follows the phase (4.20), stage 2 takes the nearest sample, and the stages, taps, weights and finish are the run's above.  One
 * rule is new: a SAMPLED full pixel whose own sample the guides accept with a weight above 0 is written by selection as that
 * low-resolution pixel's raw colour (variance: its raw variance, clamped to [0, 2^32]; stage 0), whatever the flags — a lattice
 * sample passes through unchanged.  Arguments, ordering and refusals as rayz_hip_upscaler_run; also RAYZ_ERR_BAD_ARG (before
 * the handle): a phase that is not below the factor. */
int rayz_hip_upscaler_run_phase(RayzUpscaler* up, const RayzUpscaleParams* params, uint32_t phase_x, uint32_t phase_y,
                                const float* d_rgb_lo, const float* d_var_rgb_lo_or_null, const RayzQueryOutputs* gbuffer_lo,
                                const RayzQueryOutputs* gbuffer_hi, float* d_rgb_out, float* d_var_rgb_out_or_null,
                                uint8_t* d_stage_out_or_null, void* hip_stream);
/* Waits for the handle's last run and returns its HIP-event times in ms: the pack launches, the reconstruction launch.
 * RAYZ_ERR_STATE before any run. */
int rayz_hip_upscaler_timing(RayzUpscaler* up, float* pack_ms_or_null, float* upscale_ms_or_null);
/* The FOOTPRINT ALBEDO of a low-resolution frame.  BUILD-DEFINED; f32 only; frames of block means only (the
 * camera of render.lowres_camera — a lattice sample is a real pixel with an albedo of its own).  A low-resolution pixel is the
 * mean over its factor x factor block of full pixels, but `gbuffer_lo->albedo` is one point sample at the block's centre, so
 * demodulating by it is off by the texture's contrast wherever the texture is finer than a low-resolution pixel.  This call
 * writes, for every low-resolution pixel, the mean of the RAW full-size albedos of its block whose `index` equals the pixel's own
 * (visited rows first, plain f32 adds, one divide: 4.24, restated bit for bit by tests/footprint_mirror.cpp); (1, 1, 1) for a
 * background pixel; `gbuffer_lo->albedo`'s own bits where no pixel of the block has that index.  The result is meant to stand in
 * for `gbuffer_lo->albedo` in a rayz_hip_upscaler_run with RAYZ_DENOISE_ALBEDO (and in the denoiser run of the low-resolution
 * frame); the run itself is unchanged and RayzUpscaleParams.flags gets no new bit.
 * The handle supplies the device, the sizes and the factor.  Of `gbuffer_lo` (h x w) and `gbuffer_hi` (height x width) only index
 * and albedo are read, and both are required.  d_albedo_lo_out: DEVICE memory, h*w*3 floats.  d_count_out_or_null: h*w bytes, the
 * number of full pixels of the block with the low-resolution pixel's index (for a background pixel: the block's background
 * pixels).  No output may overlap an input or the other output — writing in place into `gbuffer_lo->albedo` included.
 * Asynchronous on `hip_stream`; ordered after the handle's previous launch, and the handle's later launches are ordered after it
 * (one launch in flight per handle, as rayz_hip_upscaler_run).
 * RAYZ_ERR_BAD_ARG (checked before the handle, without touching a device): a null G-buffer, a null output, a G-buffer without
 * index or albedo, an output equal to an input or to the other output.  RAYZ_ERR_STATE: a bad handle.  RAYZ_ERR_BAD_ARG behind
 * it: an output overlapping an input or the other output.  Added within ABI 5 (additive). */
int rayz_hip_upscaler_footprint_albedo(RayzUpscaler* up, const RayzQueryOutputs* gbuffer_lo, const RayzQueryOutputs* gbuffer_hi,
                                       float* d_albedo_lo_out, uint8_t* d_count_out_or_null, void* hip_stream);
/* Waits for the handle's last footprint call and returns its launch's HIP-event time in ms.  Its events are its own:
 * rayz_hip_upscaler_timing keeps reporting the last RUN whatever footprint calls came in between.  RAYZ_ERR_STATE before any
 * footprint call. */
int rayz_hip_upscaler_footprint_timing(RayzUpscaler* up, float* ms);
int rayz_hip_upscaler_destroy(RayzUpscaler* up);

/* ---- temporal accumulation: reproject the history across camera moves -----------------------------
 * BUILD-DEFINED: the temporal stage of SVGF (Schied et al. 2017) for a caller that keeps a scene in device memory and moves the
 * camera.  A step takes the current frame (WHOLE f32 frame in DEVICE memory), its per-channel variance
 * (rayz_hip_progressive_noise_rgb) and the G-buffer a rayz_hip_scene_query_camera call of F32 precision filled for the same
 * camera; every pixel's first-hit point is projected into the PREVIOUS step's camera, the four history pixels around that position
 * are accepted where they are the same surface (same hittable, normals within `normal_cos_min`, points within `max_rel_dist` of
 * the distance to the previous camera), and the current frame is blended into their interpolated mean by sample count:
 * alpha = max(spp / (history samples + spp), alpha_min).  The variance of the blended mean is carried along, so the outputs go
 * straight into rayz_hip_denoiser_run_guided.  A camera equal to the previous step's byte for byte is a STATIC step: every pixel
 * takes its own history, no projection.  The arithmetic is a contract (§4.15, the rules of §4.11), restated bit for bit by
 * tests/temporal_mirror.cpp.  Added in ABI 5 (additive: no existing symbol changed); it changes no image any other entry point
 * produces.
 * Limits of this version: the unfiltered accumulated colour is the history unless the caller feeds a filtered one back, which only a
 * moments handle takes (rayz_hip_temporal_track_feedback, rayz_hip_temporal_feedback below; the plain step has no such mode);
 * no motion vectors — the guides are first-hit, time-0 guides, so a moving sphere is matched where it is at time 0 and its blur is
 * carried as if painted on it; reflections and refractions are not reprojected (a mirror's image is carried on the mirror's
 * surface); whole frames only (rows of a shard are not image neighbours: gather first, as for the denoiser); f32 only; no switch
 * of the `rayz` command line. */
typedef struct RayzTemporal RayzTemporal; /* opaque: two history buffers (ping-pong) for one frame size on one device + the last camera */

#define RAYZ_TEMPORAL_DEFAULT_ALPHA_MIN 0.05       /* these four: PROVISIONAL until DESIGN.md §6's measurement; parameters, not contract */
#define RAYZ_TEMPORAL_DEFAULT_N_MAX 65536.0
#define RAYZ_TEMPORAL_DEFAULT_NORMAL_COS_MIN 0.9
#define RAYZ_TEMPORAL_DEFAULT_MAX_REL_DIST 0.05

typedef struct RayzTemporalParams {
    double alpha_min;      /* in [0, 1]: the least weight of the current frame; 0 = the running sample-weighted mean, 1 = no history */
    double n_max;          /* >= 1 (+inf allowed): the history length, in samples, is capped here */
    double normal_cos_min; /* in [-1, 1]: a history pixel is accepted if dot(its normal, the current normal) >= this */
    double max_rel_dist;   /* > 0: .. and if its point lies within this fraction of the current point's distance to the previous camera */
} RayzTemporalParams;      /* all four are used as f32 */

/* device < 0: the default device (RAYZ_ERR_NO_DEVICE before rayz_hip_init); otherwise creates that device's context if needed.
 * RAYZ_ERR_BAD_ARG: a zero size, or width*height > RAYZ_DENOISE_MAX_PIXELS.  The handle owns 128 bytes per pixel. */
int rayz_hip_temporal_create(int device, uint32_t width, uint32_t height, RayzTemporal** out);
/* One frame.  d_rgb_in, d_var_rgb, d_rgb_out, d_var_out: DEVICE memory, height*width*3 floats each; d_length_out_or_null:
 * height*width floats, the history length in samples after the step (spp where no history was found).  d_rgb_out == d_rgb_in and
 * d_var_out == d_var_rgb are allowed (a pixel reads only its own current values).  `gbuffer`: index, normal and point are
 * required, the other fields are ignored.  `camera`: the camera the frame and the G-buffer were made with; `spp`: the frame's
 * samples per pixel — render every frame in at least 2 chunks, or its variance is +inf, which is carried as 2^32 (or use
 * the moments mode below, which takes the variance from the history: rayz_hip_temporal_step_moments).
 * params_or_null == NULL: all defaults.  The first step of a handle, and the first after rayz_hip_temporal_reset, has no
 * history: its outputs are its inputs (the variance clamped to [0, 2^32], a NaN taken as 2^32).
 * Asynchronous on `hip_stream` (NULL: the library's stream of the handle's device); the inputs must stay allocated until the step
 * has finished.  One step in flight per handle: a step first makes its stream wait, on the device, for the handle's previous
 * step (through an event of the handle's own, so the previous step's stream may have been destroyed by then; _destroy waits the
 * same way).
 * RAYZ_ERR_BAD_ARG (checked before the handle, without touching a device): a missing pointer (only d_length_out and params may
 * be NULL); spp == 0 or spp > 2^24; alpha_min outside [0, 1]; n_max not >= 1; normal_cos_min outside [-1, 1]; max_rel_dist not
 * > 0 (a NaN fails each of these); a camera whose px_du, px_dv and px_origin - look_from have a determinant that is 0 or not
 * finite.  RAYZ_ERR_STATE: a bad handle. */
int rayz_hip_temporal_step(RayzTemporal* tm, const RayzTemporalParams* params_or_null, const RayzCameraDesc* camera, uint32_t spp,
                           const float* d_rgb_in, const float* d_var_rgb, const RayzQueryOutputs* gbuffer, float* d_rgb_out,
                           float* d_var_out, float* d_length_out_or_null, void* hip_stream);
/* Forgets the history: the next step is a first frame.  Touches no device. */
int rayz_hip_temporal_reset(RayzTemporal* tm);
/* Waits for the handle's last step and returns its HIP-event time in *ms (may be NULL: just wait).  RAYZ_ERR_STATE before any step. */
int rayz_hip_temporal_timing(RayzTemporal* tm, float* ms);
int rayz_hip_temporal_destroy(RayzTemporal* tm);

/* ---- temporal accumulation, moments mode: the variance from the history, for one-chunk frames -------
 * BUILD-DEFINED, additive within ABI 5.  A frame of one chunk (1 .. 16 spp under the automatic schedule), a one-shot
 * rayz_hip_render_device frame or a gathered multi-GPU frame has no per-pixel variance to feed rayz_hip_temporal_step.  A handle in
 * MOMENTS MODE needs none: as SVGF does, it accumulates the second moment of the colour with the same blend as the colour and
 * reports, per channel, max(m2 - c^2, 0) * W2 / (1 - W2) — W2 being the sum of the squared weights of the frames in the
 * accumulated colour, 1/W2 the effective frame count.  Where the history is too short (W2 > w2_max: a first frame, a
 * disocclusion) the variance is estimated over the CURRENT frame's 7x7 neighbourhood on the same surface (same hittable, normals
 * within normal_cos_min; fewer than min_taps accepted taps: 2^32, "trust the guides only").  The colour and the history length of a
 * moments step equal the plain step's bit for bit.  The arithmetic is a contract (§4.16), restated by
 * tests/temporal_moments_mirror.cpp. */
#define RAYZ_TEMPORAL_MOMENTS_DEFAULT_W2_MAX 0.25   /* these two: PROVISIONAL until DESIGN.md §6's measurement; parameters, not contract */
#define RAYZ_TEMPORAL_MOMENTS_DEFAULT_MIN_TAPS 4.0

typedef struct RayzTemporalMomentsParams {
    double w2_max;   /* in [0, 1]: the spatial estimate is taken where W2 > this (0: always; 1: never) */
    double min_taps; /* in [2, 49]: .. and needs at least this many accepted taps of the 49 */
} RayzTemporalMomentsParams; /* both are used as f32 */

/* Puts the handle into moments mode: one more 16-byte record per pixel on each ping-pong side (160 bytes per pixel instead of
 * 128).  Allowed only while the handle has no history — after _create or after rayz_hip_temporal_reset — else RAYZ_ERR_STATE; a
 * second call is RAYZ_OK and does nothing.  If the allocation fails the handle stays a plain one.  From then on the handle takes
 * _step_moments and refuses _step with RAYZ_ERR_STATE (a plain handle refuses _step_moments the same way); _reset, _timing and
 * _destroy serve both kinds. */
int rayz_hip_temporal_track_moments(RayzTemporal* tm);
/* One frame, as rayz_hip_temporal_step without the variance input.  d_var_out: height*width*3 floats, the variance of each
 * channel of d_rgb_out's accumulated mean (0 on background pixels), in [0, 2^32]; d_w2_out_or_null: height*width floats, W2 after
 * the step (1 where no history was found).  d_rgb_out == d_rgb_in is NOT allowed: neighbours read the current frame.
 * mparams_or_null == NULL: the defaults above.  RAYZ_ERR_BAD_ARG (checked before the handle, without touching a device): what
 * rayz_hip_temporal_step refuses, minus the variance input; w2_max outside [0, 1]; min_taps outside [2, 49] (a NaN fails both);
 * d_rgb_out == d_rgb_in.  RAYZ_ERR_STATE: a bad handle, or one that is not in moments mode. */
int rayz_hip_temporal_step_moments(RayzTemporal* tm, const RayzTemporalParams* params_or_null,
                                   const RayzTemporalMomentsParams* mparams_or_null, const RayzCameraDesc* camera, uint32_t spp,
                                   const float* d_rgb_in, const RayzQueryOutputs* gbuffer, float* d_rgb_out, float* d_var_out,
                                   float* d_length_out_or_null, float* d_w2_out_or_null, void* hip_stream);

/* ---- temporal accumulation, feedback of the filtered colour -------------------------------------------
 * BUILD-DEFINED, additive within ABI 5.  SVGF writes the output of its first à-trous level back as the colour history: the next
 * frame then blends into a colour that has been smoothed once, while the variance still comes from RAW moments.  A moments handle
 * that TRACKS FEEDBACK keeps, in the record a moments step writes its variance to and never reads, the raw first moment m1 — what
 * the accumulated colour would be had no feedback ever been given — reprojects and blends it exactly as the colour, and reports
 * max(m2 - m1^2, 0) * W2 / (1 - W2).  Everything else of a step is §4.16's, operation for operation; a handle that tracks
 * feedback and is never given any returns what a moments handle returns, bit for bit.  The arithmetic is a contract (§4.17),
 * restated by tests/temporal_feedback_mirror.cpp.  Per frame: _step_moments, rayz_hip_denoiser_run_guided_tap with tap_level 1 on its
 * outputs, _feedback with the tap.
 * Limits of this version: moments handles only; opt-in, no default changed; the caller chooses what to feed back. */
/* Allowed only on a handle in moments mode that has no history — after _track_moments or after rayz_hip_temporal_reset — else
 * RAYZ_ERR_STATE; a second call is RAYZ_OK and does nothing.  Allocates nothing.  From then on rayz_hip_temporal_step_moments keeps m1
 * and the handle takes rayz_hip_temporal_feedback. */
int rayz_hip_temporal_track_feedback(RayzTemporal* tm);
/* Replaces the accumulated colour of every pixel of the history the last step left with d_rgb's pixel (DEVICE memory,
 * height*width*3 floats); the history length, m1, the second moment, W2 and the guides stay.  A pixel with a channel of d_rgb that
 * is not finite keeps its colour.  The next step returns, and keeps as its colour history, the blend of its frame with this
 * colour.  A second call before the next step replaces the first.  Asynchronous on `hip_stream` (NULL: the library's stream of the
 * handle's device): it first makes its stream wait for the handle's previous work, and the next step and _destroy wait for it as
 * they wait for a step; d_rgb must stay allocated until it has finished.  rayz_hip_temporal_timing keeps reporting the last step.
 * RAYZ_ERR_BAD_ARG (checked before the handle, without touching a device): d_rgb NULL.  RAYZ_ERR_STATE: a bad handle, one that
 * does not track feedback, or one without history (before the first step, after _reset). */
int rayz_hip_temporal_feedback(RayzTemporal* tm, const float* d_rgb, void* hip_stream);

/* ---- temporal accumulation, counts step: per-pixel sample counts for sparse frames -------------------
 * BUILD-DEFINED, additive within ABI 5.  rayz_hip_temporal_step and _step_moments blend every pixel with one `spp`.  A lattice frame
 * (rayz_hip_scene_render_pixels over every f-th pixel) adds samples to one pixel in f*f and none to the rest, and an adaptive frame
 * (rayz_hip_progressive_sample_counts) a different number to each.  The COUNTS STEP is the same step with `d_counts` — DEVICE
 * memory, height*width uint32, the samples the current frame adds to each pixel, 0 allowed — in place of `spp`:
 *   - a pixel with count n > 0 blends as the scalar step does with spp = n;
 *   - a pixel with count 0 that finds history KEEPS it: colour, variance (moments: second moment and W2) are the gathered history's
 *     and the length is its length, by selection; the pixel's input colour and variance are loaded and never used, so a NaN
 *     there reaches neither the outputs nor the history;
 *   - a pixel without history takes its input as always and gets the length n; a record of length 0 holds no samples, and later
 *     steps refuse it as a tap exactly as they refuse a different surface;
 *   - the moments step's 7x7 neighbourhood counts only positions whose own count is > 0, the centre included.
 * With every count equal to one spp >= 1 a counts step returns what the scalar step returns, bit for bit; under a still camera a
 * pixel with count 0 keeps its record's colour, variance / moments and length.  Counts above 2^24 are the caller's error (they
 * are used as f32) and are not checked.  The handle gains no state: scalar and counts steps may alternate on one handle.  The
 * arithmetic is a contract (§4.23), restated by tests/temporal_counts_mirror.cpp.
 * Limits of this version: plain and moments handles only — a handle that tracks feedback refuses both with RAYZ_ERR_STATE;
 * background pixels are never accumulated, as before. */
/* rayz_hip_temporal_step with d_counts for spp.  d_rgb_out == d_rgb_in and d_var_out == d_var_rgb are still allowed.
 * RAYZ_ERR_BAD_ARG (checked before the handle, without touching a device): what rayz_hip_temporal_step refuses, minus spp; d_counts
 * NULL; d_counts equal to d_rgb_out, d_var_out or d_length_out.  RAYZ_ERR_STATE: a bad handle, or one in moments mode. */
int rayz_hip_temporal_step_counts(RayzTemporal* tm, const RayzTemporalParams* params_or_null, const RayzCameraDesc* camera,
                                  const uint32_t* d_counts, const float* d_rgb_in, const float* d_var_rgb, const RayzQueryOutputs* gbuffer,
                                  float* d_rgb_out, float* d_var_out, float* d_length_out_or_null, void* hip_stream);
/* rayz_hip_temporal_step_moments with d_counts for spp.  RAYZ_ERR_BAD_ARG: what rayz_hip_temporal_step_moments refuses, minus spp;
 * d_counts NULL; d_counts equal to d_rgb_out, d_var_out, d_length_out or d_w2_out.  RAYZ_ERR_STATE: a bad handle, one that is not
 * in moments mode, or one that tracks feedback. */
int rayz_hip_temporal_step_moments_counts(RayzTemporal* tm, const RayzTemporalParams* params_or_null,
                                          const RayzTemporalMomentsParams* mparams_or_null, const RayzCameraDesc* camera,
                                          const uint32_t* d_counts, const float* d_rgb_in, const RayzQueryOutputs* gbuffer,
                                          float* d_rgb_out, float* d_var_out, float* d_length_out_or_null, float* d_w2_out_or_null,
                                          void* hip_stream);

/* ---- temporal accumulation, resampling mode: Catmull-Rom history fetch with bilinear fallback --------
 * BUILD-DEFINED, additive within ABI 5, opt-in: a handle starts in RAYZ_TEMPORAL_RESAMPLE_BILINEAR, where every step is §4.15's as
 * before, bit for bit.  Under a camera move that is no whole number of pixels the 2x2 bilinear gather low-passes the accumulated
 * colour once per frame.  In RAYZ_TEMPORAL_RESAMPLE_CUBIC a moving step fetches the colour history (in moments mode also the
 * second moment) with a 4x4 Catmull-Rom kernel WHERE all sixteen history pixels (x0 - 1 .. x0 + 2, y0 - 1 .. y0 + 2) lie inside
 * the frame and are the same surface as the current pixel by §4.15's own acceptance test, clamps the result per channel to the
 * range of the four central taps — the negative lobes cannot ring — and uses the bilinear gather everywhere else: a static step,
 * a pixel near the frame's edge or a silhouette, a pixel whose bilinear gather was renormalised.  The variance (moments: W2) and
 * the history length are interpolated bilinearly in both modes; the blend and the stores are unchanged; a move by whole pixels
 * gives the bilinear result bit for bit.  The history's layout does not change and the handle gains no device state, so the mode
 * may be changed between any two steps, with or without history.  The arithmetic is a contract (§4.26), restated by
 * tests/temporal_cubic_mirror.cpp.
 * d_taken_or_null: DEVICE memory, height*width bytes, which the caller keeps allocated until another call replaces it (NULL: none).
 * EVERY later step of the handle, in either mode, writes one byte per pixel there: 1 where the pixel's colour history came from
 * the sixteen taps, 0 otherwise — a first frame, a static step, a background pixel, a pixel without history, one that fell back,
 * and every pixel in bilinear mode.  A step refuses a d_taken that equals one of its outputs with RAYZ_ERR_BAD_ARG.
 * Limits of this version: plain handles take cubic mode through rayz_hip_temporal_step, moments handles through
 * rayz_hip_temporal_step_moments; a handle in CUBIC mode refuses rayz_hip_temporal_step_counts and _step_moments_counts with
 * RAYZ_ERR_STATE; a handle that tracks feedback refuses set_resampling(CUBIC), and a CUBIC handle refuses
 * rayz_hip_temporal_track_feedback, both with RAYZ_ERR_STATE.
 * RAYZ_ERR_BAD_ARG (checked before the handle): a mode that is neither constant.  RAYZ_ERR_STATE: a bad handle. */
#define RAYZ_TEMPORAL_RESAMPLE_BILINEAR 0u   /* default: §4.15 as it is */
#define RAYZ_TEMPORAL_RESAMPLE_CUBIC    1u
int rayz_hip_temporal_set_resampling(RayzTemporal* tm, uint32_t mode, uint8_t* d_taken_or_null);
int rayz_hip_temporal_get_resampling(RayzTemporal* tm, uint32_t* mode);

/* ---- temporal accumulation, background mode: history for pixels whose centre ray misses the scene -----
 * BUILD-DEFINED, additive within ABI 5, opt-in: a handle starts in RAYZ_TEMPORAL_BACKGROUND_INPUT, where a pixel with index < 0
 * passes its input through as before, bit for bit.  In RAYZ_TEMPORAL_BACKGROUND_ACCUMULATE such a pixel gathers history as a hit
 * pixel does: a miss sees the sky at infinity, so its place in the previous frame depends only on how the view turned — the 3x3
 * matrix between the two cameras' pixel grids, computed on the host in f64 (look_from does not enter: the sky has no parallax).
 * Its four bilinear taps accept the history pixels that were misses themselves (no normal or distance test; in a counts step also
 * a length > 0); the weight threshold, the renormalisation, the blend and the stores are a hit pixel's.  In a counts step a
 * background pixel with count 0 that finds history keeps it, so a NaN input reaches neither the outputs nor the history.  In
 * moments mode its variance is the temporal one where it found history and W2 <= w2_max, and +0 elsewhere: the 7x7 spatial
 * estimate stays a hit pixel's.  Every pixel with index >= 0 is the INPUT-mode step bit for bit, outputs and history.
 * The history's layout does not change and the handle gains no device state, so the mode may be changed between any two steps:
 * an ACCUMULATE step reads the records an INPUT step left, and the other way round.  Plain and moments handles take it through
 * all four steps (rayz_hip_temporal_step, _step_moments, _step_counts, _step_moments_counts).  The arithmetic is a contract
 * (§4.27), restated by tests/temporal_background_mirror.cpp.
 * What it does not know: a sky pixel beside a defocused or motion-blurred silhouette has samples that hit, and those do have
 * parallax; the mode treats the pixel as sky.  That is why it is not the default.
 * Limits of this version, all RAYZ_ERR_STATE: a handle that tracks feedback refuses set_background(ACCUMULATE) and an ACCUMULATE
 * handle refuses rayz_hip_temporal_track_feedback; a handle in cubic resampling mode refuses set_background(ACCUMULATE) and an
 * ACCUMULATE handle refuses set_resampling(CUBIC) — the sky has no cubic rule yet.
 * RAYZ_ERR_BAD_ARG (checked before the handle): a mode that is neither constant.  RAYZ_ERR_STATE: a bad handle. */
#define RAYZ_TEMPORAL_BACKGROUND_INPUT      0u   /* default: every section as it is */
#define RAYZ_TEMPORAL_BACKGROUND_ACCUMULATE 1u
int rayz_hip_temporal_set_background(RayzTemporal* tm, uint32_t mode);
int rayz_hip_temporal_get_background(RayzTemporal* tm, uint32_t* mode);

/* ---- temporal accumulation, clip mode: the history's colour clamped to the current frame's neighbourhood ----
 * BUILD-DEFINED, additive within ABI 5, opt-in: a handle starts in RAYZ_TEMPORAL_CLIP_OFF, where every step is what it was, bit
 * for bit.  A step accepts a history pixel by geometry alone; nothing compares its colour with the frame it is blended into, so
 * stale radiance that passes every geometric test stays.  In RAYZ_TEMPORAL_CLIP_VARIANCE a MOVING step clamps, per channel, the
 * gathered history mean of a pixel that found history to mu +- gamma*sd before the blend, where mu and sd are the mean and the
 * unbiased sample deviation of the CURRENT frame over the pixel's 7x7 neighbourhood on the same surface — §4.16 step 4's taps,
 * acceptance and sums — wherever that neighbourhood has at least min_taps pixels.  In RAYZ_TEMPORAL_BACKGROUND_ACCUMULATE a pixel
 * with index < 0 is clipped too, against the misses of its neighbourhood.  In moments mode the history's second moment of a
 * clipped channel moves with the mean and keeps its spread about it, and a pixel that also takes the spatial estimate uses the
 * same sums.  A static step, a first frame and a pixel without history are the OFF step bit for bit: a still camera keeps
 * converging to the running mean.  gamma = +inf never clips (the OFF step bit for bit); gamma = 0 replaces the history by mu.
 * What it does not do: the history length, W2 and the plain step's carried variance ignore the clip.
 * The history's layout does not change and the handle gains no device state, so the mode may be changed between any two steps,
 * with or without history.  The arithmetic is a contract (§4.28), restated by tests/temporal_clip_mirror.cpp.
 * params_or_null: NULL takes the defaults below; both are used as f32.
 * d_clipped_or_null: DEVICE memory, height*width bytes, which the caller keeps allocated until another call replaces it (NULL:
 * none).  EVERY later step of the handle, in either mode, writes one byte per pixel there: 1 where the clip changed any channel of
 * the pixel's colour history — by as little as one ulp — and 0 elsewhere; a step that runs no clip kernel clears it on its own
 * stream.  A step refuses a d_clipped that equals one of its outputs or the handle's d_taken with RAYZ_ERR_BAD_ARG.
 * Limits of this version, all RAYZ_ERR_STATE: a handle that tracks feedback or resamples cubically refuses set_clip(VARIANCE),
 * and a VARIANCE handle refuses rayz_hip_temporal_track_feedback and set_resampling(CUBIC); a VARIANCE handle refuses
 * rayz_hip_temporal_step_counts and _step_moments_counts.
 * RAYZ_ERR_BAD_ARG (checked before the handle): a mode that is neither constant; gamma not >= 0 (+inf is allowed, a NaN is not);
 * min_taps outside [2, 49].  RAYZ_ERR_STATE: a bad handle. */
#define RAYZ_TEMPORAL_CLIP_OFF      0u   /* default: every section as it is */
#define RAYZ_TEMPORAL_CLIP_VARIANCE 1u
#define RAYZ_TEMPORAL_CLIP_DEFAULT_GAMMA    1.0   /* PROVISIONAL: parameters, not contract */
#define RAYZ_TEMPORAL_CLIP_DEFAULT_MIN_TAPS 4.0
typedef struct RayzTemporalClipParams {
    double gamma;    /* >= 0: the half-width of the box in sample deviations */
    double min_taps; /* in [2, 49]: below this many accepted neighbours the history is not clipped */
} RayzTemporalClipParams; /* used as f32 */
int rayz_hip_temporal_set_clip(RayzTemporal* tm, uint32_t mode, const RayzTemporalClipParams* params_or_null, uint8_t* d_clipped_or_null);
int rayz_hip_temporal_get_clip(RayzTemporal* tm, uint32_t* mode, RayzTemporalClipParams* params_or_null);

#ifdef __cplusplus
}
#endif
#endif /* RAYZ_HIP_H */
