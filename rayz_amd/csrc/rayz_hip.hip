// rayz_hip.hip — the C ABI of include/rayz_hip.h: scene upload, workspace, kernel launches.
//
// Replaces the body of `Tracer.render()` (src/renderer.zig:72-101 of jlucier/rayz).  A scene handle is bound to
// ONE device (its own context: stream, CU count); a process may drive several devices — one scene per device,
// rows dealt in interleaved tiles (params.shard_*) — either itself (rayz_hip_multi_*: one host thread, one stream
// per device, one RCCL gather of the row tiles to the first device) or as one process per GPU with the gather
// done by the caller (torch.distributed in bench.py).
//
// One translation unit.  This file holds the scene (layout, upload, BVH upload), the chunk schedule and the trace launch: all that
// decides what a trace kernel is launched with.  It stands on host_base.hpp and includes, at its end, one header per feature: handle,
// internals, entries.
#include "../../include/rayz_hip.h"
#include "rayz_device.hpp"
#include "chain_kernel.hpp"
#include "sampled_kernel.hpp"
#include "bvh_build.hpp"
#include "denoise.hpp"
#include "upscale.hpp"
#include "temporal_kernel.hpp"
#include "temporal_moments_kernel.hpp"
#include "temporal_feedback_kernel.hpp"
#include "temporal_cubic_kernel.hpp"
#include "noise.hpp"
#include "adaptive.hpp"
#include "sparse.hpp"
#include "temporal_modes_kernel.hpp"
#include "host_base.hpp"

using namespace rayz_dev;

namespace {

// Device copy of the scene in one precision: scan streams + pool-indexed shading tables.
template <class R> struct SceneBuffers {
    typedef typename VecOf<R>::type r4;
    DevBuf<float> stat;    // blocks of G = 4 spheres: cx[G] cy[G] cz[G] r²[G]   (scan streams: f32 for both precisions)
    DevBuf<float> movy;    // blocks of G: cx[G] cy[G] cz[G] r²[G] vy[G]
    DevBuf<f4> movg;
    DevBuf<r4> sph_pool, mat, tex, tri;
    DevBuf<u4> bvh_nodes;   // BVH traversal only (f32 planes or 16-bit plane indices, for both precisions: the box test only culls)
    bool quantized = false; // .. which: DevScene::bvh_nodes
    DevBuf<r4> bvh_leaf;
    uint32_t nt_pad = 0, bvh_leaf_stride = 2, bvh_n_inner = 0;
    uint32_t n_big_leaves = 0, big_desc[4] = {0, 0, 0, 0};
    uint32_t bvh_top = 0; // inner-node records the BVH kernel copies to LDS
    rayz_bvh::PlaneGrid grid; // the grid the node records' 16-bit plane indices live on (f32 planes: origin 0, cell 1)
    double pad_S = 0; // the origin bound S the filter radii of these buffers were padded for
    bool ready = false, bvh_ready = false;
};

// The pool's own f64 records in slot order (narrow phase) + slot → pool index; shared by both precisions.
struct NarrowBuffers {
    DevBuf<d4> slot64;
    DevBuf<uint32_t> slot_pool;
    DevBuf<uint32_t> real_slots; // the slots that hold a sphere (not a pad), ascending: what primary_lists_kernel loops over
    DevBuf<d4> bvh_sph64; // leaf order (BVH traversal only)
    uint32_t ns_pad = 0, ny_pad = 0, ng_pad = 0;
    uint32_t n_real = 0; // entries of real_slots
    // the slab's cells (slab_cells.hpp): a fact of the pool and its slots alone, planned with them and uploaded with
    // slot64; cell_grid.nx = 0: the scene has none
    rayz_cells::CellGrid cell_grid{};
    std::vector<uint32_t> cell_table_host;
    DevBuf<uint32_t> cell_table;
    size_t cell_members = 0;
    // slot order of the static (0) and mov-Y (1) classes: plane runs first (rayz_plane::plan_runs), then the loose spheres
    std::vector<PlaneRun> runs[2];
    std::vector<std::vector<uint32_t>> run_members[2]; // pool indices of each run
    std::vector<uint32_t> loose[2];
    uint32_t plane_slots[2] = {0, 0};
    // speed buckets of each mov-Y run (rayz_plane::plan_buckets): the run's slot order is its buckets' members, its other
    // members, its pads
    std::vector<rayz_plane::RunBuckets> buckets;
    // the basis one scan of these slots is cheaper in (rayz_plane::cheaper_scan_form): a fact of the layout, priced with it
    uint32_t scan_form = rayz_plane::kScanFormXZ;
    // one-radius sets (rayz_plane::plan_sets) of each class: a static run's, or a speed bucket's; a run's or bucket's slot order
    // is its sets' members, then what no set took.  old_first: the first slot the old form still tests, of each run and bucket
    std::vector<rayz_plane::ClassSet> sets[2];
    std::vector<uint32_t> run_old_first[2], bucket_old_first;
    bool planned = false, ready = false, bvh_ready = false;
};

// A shard's primary lists (primary_lists.hpp) and whether they hold the lists of their owner's camera and params: a
// scene's are rebuilt by every one-shot render that uses them, a progressive handle's are built by its first pass.
struct PrimaryLists {
    DevBuf<uint32_t> buf;
    bool built = false;
};

uint32_t round_up(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }

// LDS of the traversal stacks of `lanes` lanes walking a tree of depth `depth` (sized from the tree at hand: a shallow one does not cap
// the occupancy): a u32 per level below the root (nearer child first: never two entries per level) + a guard row (reads at index −1).
size_t bvh_stack_bytes(uint32_t depth, uint32_t lanes) { return ((size_t)depth + 3) * lanes * sizeof(uint32_t); }

// ---- chunk schedule: which samples of a pixel are summed together ------------------------------
// params.chunk_spp != 0: uniform chunks of that many samples (the last one shorter).  0 = automatic: frames of fewer
// than 2^19 pixels, or fewer than 64 samples per pixel, use uniform chunks of 16; larger renders use chunks of C samples
// while at least 2 C remain, and split the rest by halving down to 16 (.. C, C/2, C/4, .., 16, 16): the work queue — which
// hands out chunk 0 of every pixel, then chunk 1, .. — ends in SHORT items, so no lane is left with a long item while the
// others have run dry.  C (auto_chunk) is sized for the frame being DEALT TO 8 GPUs (round 4): no work item larger than 1/8
// of what a lane of a 2^18-lane GPU gets of an 8-way deal, C = pixels · spp / 2^24 held to [64, 256] (a power of two, at most
// spp / 2) — 64 for 1920x1080x1024, 256 for 3840x2160x4096.  Measured (profiles/r04/multi/): with C = 256 one GPU's share of
// the 1080p frame runs at 80 - 87 % of the whole-frame rate (≈1 pixel per lane: three items of a quarter of a lane's work
// each, nothing left to balance with), with 64 at 94 %; the whole frame on ONE GPU changes by +1.0 % (flat list) / −1.2 % (BVH).
// The price is partial sums: 18 per pixel instead of 8 at 1024 spp.  Depends on the full frame's size, never on the shard or
// the GPU count: the image is the same for every deal.
uint64_t pow2floor(uint64_t v) { // the largest power of two <= max(v, 1)
    uint64_t r = 1;
    while (r <= v / 2) r *= 2;
    return r;
}
bool uniform_chunks(const RayzRenderParams* p) {
    return p->chunk_spp != 0 || (uint64_t)p->width * p->height < (1ull << 19) || p->samples_per_px < 64;
}
uint32_t auto_chunk(uint64_t pixels, uint32_t spp) {
    const uint64_t share = pixels >= (1ull << 32) ? 256 : (pixels * spp) >> 24;
    long long cap = (long long)pow2floor(std::min<uint64_t>(256, std::max<uint64_t>(64, share)));
#ifdef RAYZ_EXPERIMENTS // tools/chunk_cap_sweep.py only: CHANGES the summation tree (the oracle does not follow it)
    cap = tuning(RAYZ_DEBUG_CHUNK_CAP, cap);
#endif
    return (uint32_t)std::min<uint64_t>((uint64_t)cap, pow2floor(spp / 2));
}
void chunk_schedule(const RayzRenderParams* p, std::vector<uint32_t>& starts) {
    const uint32_t spp = p->samples_per_px;
    starts.clear();
    starts.push_back(0);
    if (uniform_chunks(p)) {
        const uint32_t c = p->chunk_spp ? p->chunk_spp : 16u;
        for (uint64_t s0 = c; s0 < spp; s0 += c) starts.push_back((uint32_t)s0);
        starts.push_back(spp);
        return;
    }
    const uint32_t C = auto_chunk((uint64_t)p->width * p->height, spp);
    uint32_t at = 0, rem = spp;
    while (rem >= 2 * C) at += C, rem -= C, starts.push_back(at);
    while (rem > 16) {
        const uint32_t c = std::max(16u, (uint32_t)pow2floor(rem / 2));
        at += c, rem -= c, starts.push_back(at);
    }
    if (rem) starts.push_back(at + rem);
}

// Number of chunks of that schedule, without building it (a pixel may have at most kMaxChunksPerPx: the table is a host
// vector, a device array and the divisor of every work item's index).
constexpr uint64_t kMaxChunksPerPx = 1ull << 20;
uint64_t chunk_count(const RayzRenderParams* p) {
    const uint64_t spp = p->samples_per_px;
    if (uniform_chunks(p)) {
        const uint64_t c = p->chunk_spp ? p->chunk_spp : 16u;
        return (spp + c - 1) / c;
    }
    // the automatic schedule, counted exactly by chunk_schedule's own rule (the full chunks in closed form, the halving
    // tail by its ≤ 10 steps): `spp / 256 + 8` undercounted tails of 256 .. 511 samples by one (spp = 497: 10 chunks)
    const uint64_t C = auto_chunk((uint64_t)p->width * p->height, (uint32_t)spp);
    uint64_t n = spp >= 2 * C ? (spp - 2 * C) / C + 1 : 0, rem = spp - n * C;
    while (rem > 16) rem -= std::max<uint64_t>(16, pow2floor(rem / 2)), ++n;
    return n + (rem ? 1 : 0);
}

double norm3(const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// ---- conservative reject filter ---------------------------------------------------------------
// The scan and the BVH leaves test r_pad² − p1² − p2² ≥ 0 in R with r_pad = r + E, E = 32·u·(|c| + |v| + r + S):
// u = unit roundoff of R, S = a bound on |o| of every ray the render can produce (camera lens, hit points on any
// hittable).  The padded square is rounded UP to R.  Candidates are decided by the f64 narrow phase, so the padding
// changes no image — it only guarantees that no sphere with an f64 discriminant ≥ 0 is filtered out.
template <class R> constexpr double unit_roundoff() { return sizeof(R) == 4 ? 5.9604644775390625e-08 : 1.1102230246251565e-16; }
// The scan streams' filter runs in f32 for both precisions.  For R = double the ray reaches it narrowed to f32 (origin,
// unit direction, time: ≤ u·S + u·(|c| + S) + u·|v| more on the line's distance to the centre), so its pad is 40u, not 32u.
template <class R> float pad_radius2_scan(const RayzSphere& q, double S) {
    const double E = (sizeof(R) == 4 ? 32.0 : 40.0) * unit_roundoff<float>() *
                     (norm3(q.center) + norm3(q.velocity) + std::fabs(q.radius) + S);
    const double rp = std::fabs(q.radius) + E;
    return rayz_bvh::roundUp<float>(rp * rp);
}
// A speed bucket's sphere (rayz_plane::plan_buckets) is tested as the sphere of velocity (0, v0, 0) and radius
// r + h, h ≥ |vy − v0|: at every time in [0, 1] that sphere contains the pool's own, so a line that meets the pool's sphere
// meets it, and the pad rule above holds for it as for any sphere (its |v| is at most |v| + h).  h is taken against the
// pool's f64 speed and the f32 one the buckets were cut by, rounded up.
template <class R> float pad_radius2_bucket(const RayzSphere& q, double S, float v0) {
    const double h = rayz_plane::bucket_h(q.velocity[1], v0);
    const double E = (sizeof(R) == 4 ? 32.0 : 40.0) * unit_roundoff<float>() *
                     (norm3(q.center) + norm3(q.velocity) + h + std::fabs(q.radius) + h + S);
    const double rp = std::fabs(q.radius) + h + E;
    return rayz_bvh::roundUp<float>(rp * rp);
}
double scene_origin_bound(const RayzScene* s);
double camera_origin_bound(const RayzCameraDesc* c) { return norm3(c->look_from) + norm3(c->defocus_u) + norm3(c->defocus_v); }

} // namespace

struct RayzScene {
    int device = -1; // HIP ordinal this scene's buffers live on; bound at creation (_on) or at the first render
    double origin_bound = -1; // max |hit point| over the pool (lazily)
    std::vector<RayzSphere> spheres;
    std::vector<RayzMaterial> materials;
    std::vector<RayzTexture> textures;
    std::vector<RayzTriangle> triangles;
    SceneBuffers<float> f32;
    SceneBuffers<double> f64;
    NarrowBuffers narrow;
    std::vector<uint32_t> cls[3]; // pool indices by velocity class: static, mov-Y, mov-G (pool order inside)
    rayz_bvh::FlatBvh bvh;        // host build of the reference's BVH (lazily, first BVH render / export)
    bool bvh_built = false;
    rayz_bvh::FlatBvh bvh_dev;    // the tree the GPU walks: the same build with the oversized hittables kept out (bvh_build.hpp)
    bool bvh_dev_built = false;
    DevBytes partial;               // chunk sums, grow-only
    DevBuf<uint32_t> chunk_start;   // device copy of the chunk schedule of the last render, grow-only
    std::vector<uint32_t> chunk_start_host;
    DevBuf<unsigned long long> counters; // [0] queue head, [1] segments
    DevEvent ev0, ev1;
    hipStream_t last_stream = nullptr;
    bool rendered = false, last_bvh = false;
    int last_experiment = 0; // the last render's BvhLaunchPlan::experiment (0: a product kernel)
    uint32_t scan_form = rayz_plane::kScanFormAuto; // rayz_hip_scene_set_scan_form: auto = the layout's own (narrow.scan_form)
    uint32_t primary_mode = RAYZ_PRIMARY_LISTS_AUTO; // rayz_hip_scene_set_primary_lists
    PrimaryLists primary;                            // the one-shot renders' lists: rebuilt by every render that uses them
    uint32_t cells_mode = RAYZ_CELL_LISTS_AUTO;      // rayz_hip_scene_set_cell_lists
    RayzRenderStats last{};
    // sparse renders (rayz_hip_scene_render_pixels, sparse_render.hpp): the check's count, and the call's events — [0], [1] around
    // its check, trace and resolve, which rayz_hip_scene_sync times when the last render was one (last_sparse); [2], [3] the trace
    DevBuf<uint32_t> sparse_bad;
    DevEvent sparse_ev[4];
    bool last_sparse = false;
    // ray queries (rayz_hip_scene_query*): their own counters and events, so that rayz_hip_scene_sync keeps reporting the last render
    DevBuf<unsigned long long> q_counters; // [0] batch head, [1] segments (chain calls), [2] node tests, [3] sphere tests, [31] LDS flag,
                                           // [kQueryBoundBase + k·kQueryBoundStride] the bound check's four words
    DevEvent q_ev0, q_ev1;
    hipStream_t q_stream = nullptr;
    bool queried = false, q_bvh = false, q_chain = false; // (q_chain: the query in flight is a chain call, chain.hpp)
    DevBuf<unsigned long long> q_chain_stores; // a chain call's output pointers (ChainStores, chain_kernel.hpp), which its kernel reads from device memory
    bool q_sampled = false;      // the query in flight is a sampled call (sampled.hpp)
    DevBytes q_sampled_sums;     // .. and its workspace: the sums of every pixel between two samples (sampled_kernel.hpp)
    RayzRenderStats q_last{};
    // The members free themselves; what is left is to wait for the scene's last launch first.
    ~RayzScene() {
        if (device < 0 || !last_stream) return;
        DeviceScope scope(device);
        (void)hipStreamSynchronize(last_stream);
    }
};

namespace {

template <class R> SceneBuffers<R>& buffers_of(RayzScene& s) {
    if constexpr (sizeof(R) == 4) return s.f32;
    else return s.f64;
}

// Every scattered ray starts at a hit point: on a sphere (|p| ≤ |c| + |v| + r, t ∈ [0,1)) or on a triangle.
double scene_origin_bound(const RayzScene* s) {
    double S = 0;
    for (const RayzSphere& q : s->spheres) S = std::max(S, norm3(q.center) + norm3(q.velocity) + std::fabs(q.radius));
    for (const RayzTriangle& q : s->triangles) S = std::max({S, norm3(q.v0), norm3(q.v1), norm3(q.v2)});
    return S * (1.0 + 1e-3);
}

// velocity class of a pool sphere: 0 static, 1 v = (0, vy, 0), 2 anything else
int velocity_class(const RayzSphere& q) {
    const bool x = q.velocity[0] != 0, y = q.velocity[1] != 0, z = q.velocity[2] != 0;
    if (!x && !y && !z) return 0;
    return (!x && !z) ? 1 : 2;
}

void classify(RayzScene* s) {
    for (auto& c : s->cls) c.clear();
    for (uint32_t i = 0; i < s->spheres.size(); ++i) s->cls[velocity_class(s->spheres[i])].push_back(i);
}

// scanned length of a stream (whole group pairs) and its allocated length (+ two spare groups for the prefetch)
uint32_t scan_len(size_t n, uint32_t group) { return round_up((uint32_t)n, 2 * group); }
uint32_t stream_len(size_t n, uint32_t group) { return scan_len(n, group) + 2 * group; }

// Every sphere's slot: place(slot, pool index) over the three classes.  A run's members fill its first slots; its pads keep slot_pool
// 0 (never a candidate: r² = -inf).
template <class F> void for_each_slot(const RayzScene* s, F&& place) {
    const NarrowBuffers& nb = s->narrow;
    const size_t class0[2] = {0, nb.ns_pad};
    for (int c = 0; c < 2; ++c) {
        for (size_t j = 0; j < nb.runs[c].size(); ++j)
            for (size_t k = 0; k < nb.run_members[c][j].size(); ++k) place(class0[c] + nb.runs[c][j].first + k, nb.run_members[c][j][k]);
        for (size_t k = 0; k < nb.loose[c].size(); ++k) place(class0[c] + nb.plane_slots[c] + k, nb.loose[c][k]);
    }
    for (size_t k = 0; k < s->cls[2].size(); ++k) place((size_t)nb.ns_pad + nb.ny_pad + k, s->cls[2][k]);
}

// The slot layout of the pool (host only): classes, plane runs, speed buckets, slot counts — and with them the scan's price
// under either basis.
void plan_slots(RayzScene* s) {
    NarrowBuffers& nb = s->narrow;
    if (nb.planned) return;
    classify(s);
    // slot numbering is shared by both precisions: pad to the larger (f32) group size.  Static and mov-Y: plane runs,
    // each padded to whole group pairs, then the loose spheres
    static_assert(kStaticGroup == kMovYGroup, "one run padding for both classes");
    for (int c = 0; c < 2; ++c)
        nb.plane_slots[c] = rayz_plane::plan_runs(s->cls[c], [&](uint32_t pool) { return (float)s->spheres[pool].center[1]; },
                                                  kStaticGroup, nb.runs[c], nb.run_members[c], nb.loose[c]);
    nb.buckets.clear();
    for (std::vector<uint32_t>& m : nb.run_members[1]) {
        nb.buckets.push_back(rayz_plane::plan_buckets(
            m, [&](uint32_t pool) { return (float)s->spheres[pool].velocity[1]; },
            [&](uint32_t pool) { return std::fabs(s->spheres[pool].radius); }, kMovYGroup));
        m = nb.buckets.back().order; // slot order from here on
    }
    // one-radius sets of each static run and of each speed bucket (rayz_plane::plan_class_sets): slot order from here on
    auto rad = [&](uint32_t pool) { return std::fabs(s->spheres[pool].radius); };
    auto vy64 = [&](uint32_t pool) { return s->spheres[pool].velocity[1]; };
    std::vector<uint32_t> none;
    rayz_plane::plan_class_sets(nb.runs[0], nb.run_members[0], nullptr, rad, vy64, nb.sets[0], nb.run_old_first[0], none);
    rayz_plane::plan_class_sets(nb.runs[1], nb.run_members[1], &nb.buckets, rad, vy64, nb.sets[1], nb.run_old_first[1], nb.bucket_old_first);
    nb.ns_pad = nb.plane_slots[0] + scan_len(nb.loose[0].size(), kStaticGroup);
    nb.ny_pad = nb.plane_slots[1] + scan_len(nb.loose[1].size(), kMovYGroup);
    nb.ng_pad = scan_len(s->cls[2].size(), kMovGGroup);
    const uint32_t class_slots[2] = {nb.ns_pad, nb.ny_pad};
    nb.scan_form = rayz_plane::cheaper_scan_form(rayz_plane::scan_slots(nb.plane_slots, class_slots, nb.buckets, nb.ng_pad));
    nb.planned = true;
    // the cells, over the slots just planned (every gate but AUTO's member count, which scene_cell_lists applies)
    std::vector<rayz_cells::SphereIn> in(s->spheres.size());
    for_each_slot(s, [&](size_t slot, uint32_t pool) {
        const RayzSphere& q = s->spheres[pool];
        rayz_cells::SphereIn& e = in[pool];
        for (int k = 0; k < 3; ++k) e.c[k] = q.center[k], e.v[k] = q.velocity[k];
        e.r = q.radius;
        e.slot = (uint32_t)slot;
    });
    rayz_cells::CellTable t = rayz_cells::build_cells(in, !s->triangles.empty(), 1u);
    nb.cell_grid = t.grid;
    nb.cell_table_host = std::move(t.table);
    nb.cell_members = 0;
    for (uint8_t m : t.member) nb.cell_members += m;
}

int upload_narrow_body(RayzScene* s) {
    NarrowBuffers& nb = s->narrow;
    plan_slots(s);
    const size_t slots = (size_t)nb.ns_pad + nb.ny_pad + nb.ng_pad;
    std::vector<d4> slot64(2 * slots, d4{0, 0, 0, 0});
    std::vector<uint32_t> slot_pool(slots, 0u);
    std::vector<uint32_t> real_slots;
    for_each_slot(s, [&](size_t slot, uint32_t pool) {
        real_slots.push_back((uint32_t)slot);
        const RayzSphere& q = s->spheres[pool];
        slot64[2 * slot] = d4{q.center[0], q.center[1], q.center[2], q.radius * q.radius}; // radius * radius in f64, src/geom.zig:45
        slot64[2 * slot + 1] = d4{q.velocity[0], q.velocity[1], q.velocity[2], 0.0};
        slot_pool[slot] = pool;
    });
    HIP_TRY(nb.slot64.upload(slot64));
    if (nb.cell_grid.nx) HIP_TRY(nb.cell_table.upload(nb.cell_table_host));
    HIP_TRY(nb.slot_pool.upload(slot_pool));
    std::sort(real_slots.begin(), real_slots.end());
    HIP_TRY(nb.real_slots.upload(real_slots));
    nb.n_real = (uint32_t)real_slots.size();
    nb.ready = true;
    return RAYZ_OK;
}

// A failed upload leaves nothing behind: the partly filled buffer set is replaced by a fresh one, so a retry starts clean.
int upload_narrow(RayzScene* s) {
    if (s->narrow.ready) return RAYZ_OK;
    const int rc = upload_narrow_body(s);
    if (rc != RAYZ_OK) s->narrow = NarrowBuffers{};
    return rc;
}

template <class R> int upload_body(RayzScene* s, SceneBuffers<R>& b) {
    typedef typename VecOf<R>::type r4;
    RAYZ_TRY(upload_narrow(s));
    auto rec = [&](uint32_t pool) { // w = the PADDED r² of the conservative filter
        const RayzSphere& q = s->spheres[pool];
        return r4{(R)q.center[0], (R)q.center[1], (R)q.center[2], (R)pad_radius2_scan<R>(q, b.pad_S)};
    };
    // static / mov-Y streams (f32 for both precisions): blocks of G spheres, SoA inside a block (field f of sphere k of
    // block g at g·W·G + f·G + k).  After the head (kPlaneHeader words: layout and run table, device_types.hpp), the plane
    // section — its runs at their slots, W = F − 1 fields (no cy: the run table holds it), two spare groups — then the
    // loose section, W = F, two spare groups.  Pad spheres {0, (0,) 0, r² = -inf, vy = 0}.  The field offsets are the device
    // forms' own (PackedGroup in flat_scan.hpp): every sphere and pad below is placed by the form's put().
    const float ninf32 = -std::numeric_limits<float>::infinity();
    auto rec32 = [&](uint32_t pool) { // r2 = the PADDED r² of the conservative filter
        const RayzSphere& q = s->spheres[pool];
        return BlockSphere<float>{(float)q.center[0], (float)q.center[1], (float)q.center[2], pad_radius2_scan<R>(q, b.pad_S), (float)q.velocity[1]};
    };
    // every scan the device runs over these streams stays inside its section's spare groups (rayz_plane::scan_reach)
    static_assert(rayz_plane::kScanSpareGroups == 2, "the sections below end in two spare groups");
    bool reach_ok = true;
    auto reach = [&](uint32_t first, uint32_t end, uint32_t group, uint32_t section_slots) {
        reach_ok = reach_ok && rayz_plane::scan_reach(first, end, group) <= section_slots;
    };
    auto blocks = [&](auto cls, uint32_t class_slots) { // cls: the class as a constant; its forms place the fields (PackedGroup::put)
        constexpr int c = decltype(cls)::value;
        typedef ScanGroup<float, c> Loose;
        typedef ScanGroup<float, c + 3> Run;
        typedef ScanGroup<float, 5> Bucket;
        const NarrowBuffers& nb = s->narrow;
        const uint32_t G = group_size<float>(), F = Loose::kWords, P = Run::kWords;
        const uint32_t n_plane = nb.plane_slots[c] + 2 * G, n_loose = class_slots - nb.plane_slots[c] + 2 * G;
        for (const PlaneRun& r : nb.runs[c]) reach(r.first, r.end, G, n_plane); // (a mov-Y run's remainder starts later, ends there)
        reach(0, class_slots - nb.plane_slots[c], G, n_loose);
        std::vector<float> v(kPlaneHeader + (size_t)n_plane * P + (size_t)n_loose * F, 0.0f);
        const uint32_t head[4] = {(uint32_t)nb.runs[c].size(), nb.plane_slots[c], 0u, 0u}; // the stream's head (device_types.hpp)
        std::memcpy(v.data(), head, sizeof(head));
        std::memcpy(v.data() + 4, nb.runs[c].data(), nb.runs[c].size() * sizeof(PlaneRun));
        float* const plane = v.data() + kPlaneHeader;
        float* const loose = plane + (size_t)n_plane * P;
        for (uint32_t k = 0; k < n_plane; ++k) Run::put(plane, k);
        for (uint32_t k = 0; k < n_loose; ++k) Loose::put(loose, k);
        for (size_t j = 0; j < nb.runs[c].size(); ++j)
            for (size_t m = 0; m < nb.run_members[c][j].size(); ++m) {
                const uint32_t pool = nb.run_members[c][j][m], k = nb.runs[c][j].first + (uint32_t)m;
                Run::put(plane, k, rec32(pool));
            }
        for (size_t k = 0; k < nb.loose[c].size(); ++k) Loose::put(loose, k, rec32(nb.loose[c][k]));
        // The set section (device_types.hpp), behind everything the stream held before it: {sets, copied bucket records, 0, 0, the
        // first old-form slot of each run}, the set table, the bucket table once more with each bucket's first old-form slot, the
        // sets' 2-field blocks cx[G'] cz[G'] back to back, two spare groups.  Nothing in front of it changes.
        auto append_sets = [&](std::vector<float>& v, std::vector<rayz_plane::SpeedBucket> table) {
            typedef ScanGroup<float, 6> Set;
            const uint32_t GS = Set::G;
            const size_t sec = rayz_plane::set_section((uint32_t)v.size());
            std::vector<rayz_plane::RadiusSet> sets;
            uint32_t set_slots = 0;
            for (const rayz_plane::ClassSet& h : nb.sets[c]) set_slots += h.count;
            const size_t blocks0 = rayz_plane::set_section((uint32_t)(sec + rayz_plane::kSetHeader + 8 * (nb.sets[c].size() + table.size())));
            v.resize(blocks0 + Set::kWords * (size_t)(set_slots + 2 * GS), 0.0f);
            float* const blk = v.data() + blocks0;
            uint32_t at = 0;
            for (const rayz_plane::ClassSet& h : nb.sets[c]) {
                for (uint32_t k = 0; k < h.count; ++k) {
                    const RayzSphere& q = s->spheres[nb.run_members[c][h.run][h.first - nb.runs[c][h.run].first + k]];
                    Set::put(blk, at + k, {(float)q.center[0], 0.0f, (float)q.center[2], 0.0f, 0.0f});
                }
                const float R2 = rayz_plane::class_set_r2(h, nb.runs[c][h.run], nb.run_members[c][h.run], [&](uint32_t pool) { return s->spheres[pool].center; },
                                                          [&](uint32_t pool) { return s->spheres[pool].velocity; }, b.pad_S, sizeof(R) == 8);
                reach(at, at + h.count, GS, set_slots + 2 * GS);
                sets.push_back({h.first, h.first + h.count, (uint32_t)blocks0 + Set::kWords * at - Set::kWords * h.first, R2, nb.runs[c][h.run].cy, h.v0, {0u, 0u}});
                at += h.count;
            }
            for (size_t q = 0; q < table.size(); ++q) table[q].first = nb.bucket_old_first[q];
            uint32_t hdr[rayz_plane::kSetHeader] = {(uint32_t)sets.size(), (uint32_t)table.size(), 0u, 0u, 0u, 0u, 0u, 0u};
            for (size_t j = 0; j < nb.run_old_first[c].size(); ++j) hdr[4 + j] = nb.run_old_first[c][j];
            std::memcpy(v.data() + sec, hdr, sizeof(hdr));
            if (!sets.empty()) std::memcpy(v.data() + sec + rayz_plane::kSetHeader, sets.data(), sets.size() * sizeof(rayz_plane::RadiusSet));
            if (!table.empty()) std::memcpy(v.data() + sec + rayz_plane::kSetHeader + 8 * sets.size(), table.data(), table.size() * sizeof(rayz_plane::SpeedBucket));
        };
        if (c != 1) {
            // (the device finds the set section from the head's two slot counts, scan_plane_class)
            reach_ok = reach_ok && v.size() == kPlaneHeader + (size_t)P * (nb.plane_slots[c] + 2 * G) + (size_t)F * (class_slots - nb.plane_slots[c] + 2 * G);
            append_sets(v, {});
            return v;
        }
        // mov-Y only: the bucket section (device_types.hpp) — per run the first slot of its 4-field remainder, the bucket table,
        // the buckets' 3-field blocks cx[G] cz[G] r2b[G] back to back, two spare groups.  Head words 2 and 3: where, how many.
        // (The buckets' slots keep their places in the plane section above, unused.)
        std::vector<rayz_plane::SpeedBucket> table;
        uint32_t rem_first[kMaxPlaneRuns] = {0, 0, 0, 0}, bucket_slots = 0;
        for (size_t j = 0; j < nb.runs[1].size(); ++j) {
            uint32_t at = nb.runs[1][j].first;
            for (size_t q = 0; q < nb.buckets[j].count.size(); ++q) {
                table.push_back(rayz_plane::SpeedBucket{nb.buckets[j].v0[q], nb.runs[1][j].cy, at, at + nb.buckets[j].count[q], bucket_slots, (uint32_t)j, {0u, 0u}});
                at += nb.buckets[j].count[q], bucket_slots += nb.buckets[j].count[q];
            }
            rem_first[j] = at;
        }
        const size_t section = (v.size() + 15) / 16 * 16; // 64-byte aligned, as the blocks are
        const size_t blocks0 = section + kBucketHeader + table.size() * (sizeof(rayz_plane::SpeedBucket) / sizeof(float));
        v.resize(blocks0 + Bucket::kWords * (size_t)(bucket_slots + 2 * G), 0.0f);
        float* const bk = v.data() + blocks0;
        for (uint32_t k = 0; k < bucket_slots + 2 * G; ++k) Bucket::put(bk, k);
        for (rayz_plane::SpeedBucket& t : table) {
            const uint32_t at = t.base; // the bucket's first slot of the section
            for (uint32_t k = t.first; k < t.end; ++k) {
                const uint32_t pool = nb.run_members[1][t.run][k - nb.runs[1][t.run].first], sk = at + (k - t.first);
                const RayzSphere& q = s->spheres[pool];
                Bucket::put(bk, sk, {(float)q.center[0], 0.0f, (float)q.center[2], pad_radius2_bucket<R>(q, b.pad_S, t.v0), 0.0f});
            }
            reach(at, at + (t.end - t.first), G, bucket_slots + 2 * G);
            t.base = (uint32_t)blocks0 + Bucket::kWords * (at - t.first); // (>= 0: the section lies behind 4 words per plane slot)
        }
        const uint32_t where[2] = {(uint32_t)section, (uint32_t)table.size()};
        std::memcpy(v.data() + 2, where, sizeof(where));
        std::memcpy(v.data() + section, rem_first, sizeof(rem_first));
        if (!table.empty()) std::memcpy(v.data() + section + kBucketHeader, table.data(), table.size() * sizeof(rayz_plane::SpeedBucket));
        // (the device finds the set section from the bucket table, scan_plane_class: the last bucket's blocks end the old content)
        const size_t dev_end = (table.empty() ? section + kBucketHeader : table.back().base + Bucket::kWords * (size_t)table.back().end) + Bucket::kWords * 2 * G;
        reach_ok = reach_ok && dev_end == v.size();
        append_sets(v, table);
        return v;
    };
    const std::vector<float> stat = blocks(std::integral_constant<int, 0>(), s->narrow.ns_pad),
                             movy = blocks(std::integral_constant<int, 1>(), s->narrow.ny_pad);
    std::vector<f4> movg(2 * (size_t)stream_len(s->cls[2].size(), kMovGGroup), f4{0.0f, 0.0f, 0.0f, 0.0f});
    reach(0, s->narrow.ng_pad, kMovGGroup, (uint32_t)(movg.size() / 2));
    if (!reach_ok) return fail(RAYZ_ERR_STATE, "scan stream layout: a scan would load past its section's spare groups");
    for (size_t k = 0; k < movg.size(); k += 2) movg[k] = f4{0.0f, 0.0f, 0.0f, ninf32};
    for (size_t k = 0; k < s->cls[2].size(); ++k) {
        const RayzSphere& q = s->spheres[s->cls[2][k]];
        movg[2 * k] = f4{(float)q.center[0], (float)q.center[1], (float)q.center[2], pad_radius2_scan<R>(q, b.pad_S)};
        movg[2 * k + 1] = f4{(float)q.velocity[0], (float)q.velocity[1], (float)q.velocity[2], 0.0f};
    }
    // triangles: {v0, bits(material)}, {e1, 0}, {e2, 0}; edges subtracted in f64, then narrowed
    b.nt_pad = scan_len(s->triangles.size(), kTriGroup);
    std::vector<r4> tri(3 * (size_t)(b.nt_pad + kTriGroup), r4{R(0), R(0), R(0), R(0)});
    for (size_t k = 0; k < s->triangles.size(); ++k) {
        const RayzTriangle& q = s->triangles[k];
        tri[3 * k] = r4{(R)q.v0[0], (R)q.v0[1], (R)q.v0[2], Bits<R>::from(q.material)};
        tri[3 * k + 1] = r4{(R)(q.v1[0] - q.v0[0]), (R)(q.v1[1] - q.v0[1]), (R)(q.v1[2] - q.v0[2]), R(0)};
        tri[3 * k + 2] = r4{(R)(q.v2[0] - q.v0[0]), (R)(q.v2[1] - q.v0[1]), (R)(q.v2[2] - q.v0[2]), R(0)};
    }
    HIP_TRY(b.tri.upload(tri));
    std::vector<r4> sph_pool, mat, tex;
    for (uint32_t i = 0; i < s->spheres.size(); ++i) {
        const RayzSphere& q = s->spheres[i];
        sph_pool.push_back(rec(i));
        sph_pool.push_back(r4{(R)q.velocity[0], (R)q.velocity[1], (R)q.velocity[2], Bits<R>::from(q.material)});
    }
    for (const RayzMaterial& m : s->materials) {
        const R p = (R)m.param;
        mat.push_back(r4{Bits<R>::from(m.kind | (m.method << 8)), Bits<R>::from(m.texture), p, R(1) / p});
    }
    for (const RayzTexture& t : s->textures) {
        tex.push_back(r4{Bits<R>::from(t.kind), Bits<R>::from(t.even), Bits<R>::from(t.odd), (R)t.scale});
        tex.push_back(r4{(R)t.color[0], (R)t.color[1], (R)t.color[2], R(0)});
    }
    HIP_TRY(b.stat.upload(stat));
    HIP_TRY(b.movy.upload(movy));
    HIP_TRY(b.movg.upload(movg));
    HIP_TRY(b.sph_pool.upload(sph_pool));
    HIP_TRY(b.mat.upload(mat));
    HIP_TRY(b.tex.upload(tex));
    b.ready = true;
    return RAYZ_OK;
}

// `S` = the origin bound this render needs.  Buffers padded for a smaller bound are rebuilt (for twice the bound, so
// that a moving camera does not rebuild every frame); the padding changes no image.
template <class R> int upload(RayzScene* s, SceneBuffers<R>& b, double S) {
    if (b.ready && b.pad_S >= S) return RAYZ_OK;
    const bool again = b.ready;
    if (again) HIP_TRY(hipDeviceSynchronize());
    b = SceneBuffers<R>{}; // (every field: what the BVH upload fills is rebuilt with the tree, bvh_ready being false again)
    b.pad_S = again ? 2.0 * S : S;
    const int rc = upload_body<R>(s, b);
    if (rc != RAYZ_OK) b = SceneBuffers<R>{};
    return rc;
}

// The basis the scene's next flat-list render scans in.
uint32_t scene_scan_form(RayzScene* s) {
    if (s->scan_form != rayz_plane::kScanFormAuto) return s->scan_form;
    plan_slots(s);
    // .. with the one-radius sets in their own loop where the layout's form is XY and the sets are large enough to pay for their
    // section (rayz_plane::kSetPayoffSlots)
    uint64_t set_slots = 0;
    for (const auto& sets : s->narrow.sets)
        for (const rayz_plane::ClassSet& t : sets) set_slots += t.count;
    if (s->narrow.scan_form == rayz_plane::kScanFormXY && set_slots >= rayz_plane::kSetPayoffSlots) return rayz_plane::kScanFormOneRadius;
    return s->narrow.scan_form;
}

// Whether a flat-list launch of `spp` samples per pixel resolves its camera segments from primary lists: never
// with triangles (scan_triangles has no list) or without spheres; AUTO from kPrimaryMinSpheres spheres and kPrimaryMinSpp samples on.
bool scene_primary_lists(const RayzScene* s, uint32_t spp) {
    if (s->primary_mode == RAYZ_PRIMARY_LISTS_OFF || !s->triangles.empty() || s->spheres.empty()) return false;
    if (s->primary_mode == RAYZ_PRIMARY_LISTS_ON) return true;
    return s->spheres.size() >= rayz_plane::kPrimaryMinSpheres && spp >= rayz_plane::kPrimaryMinSpp;
}

// Whether one-shot and progressive flat-list renders resolve their listable segments from the slab's cells: only
// where the scene has a table (no triangle, at most kMaxOutliers outliers, a member); AUTO from kCellsMinMembers members on.
bool scene_cell_lists(RayzScene* s) {
    if (s->cells_mode == RAYZ_CELL_LISTS_OFF) return false;
    plan_slots(s);
    if (!s->narrow.cell_grid.nx) return false;
    return s->cells_mode == RAYZ_CELL_LISTS_ON || s->narrow.cell_members >= rayz_cells::kCellsMinMembers;
}

void ensure_bvh(RayzScene* s) {
    if (!s->bvh_built) {
        s->bvh = rayz_bvh::build(s->spheres, s->triangles); // replaces initHittables + bvh.build, src/renderer.zig:76-78
        s->bvh_built = true;
    }
}

void ensure_bvh_dev(RayzScene* s) {
    if (!s->bvh_dev_built) {
        // RAYZ_DEBUG_BVH_PEEL = 0 (measurement only): walk the reference's full tree
        s->bvh_dev = rayz_bvh::build(s->spheres, s->triangles, tuning(RAYZ_DEBUG_BVH_PEEL, 1) != 0, tuning(RAYZ_DEBUG_BVH_SPLIT, 0) == 0);
        s->bvh_dev_built = true;
    }
}

template <class R> int upload_bvh_body(RayzScene* s, SceneBuffers<R>& b) {
    typedef typename VecOf<R>::type r4;
    ensure_bvh_dev(s);
    const rayz_bvh::FlatBvh& t = s->bvh_dev;
    const uint32_t ns = (uint32_t)s->spheres.size();
    // leaf-order slots: the tree's hittables, then the oversized ones kept out of it
    std::vector<uint32_t> slots(t.order);
    slots.insert(slots.end(), t.big.begin(), t.big.end());
    b.n_big_leaves = 0;
    for (size_t k = 0; k < t.big.size(); k += 2) {
        const uint32_t first = (uint32_t)(t.order.size() + k), count = (uint32_t)std::min<size_t>(2, t.big.size() - k);
        uint32_t desc = (first << 4) | count;
        for (uint32_t j = 0; j < count; ++j)
            if (t.big[k + j] >= ns) desc |= 1u << (2 + j);
        b.big_desc[b.n_big_leaves++] = desc;
    }
    if (!s->narrow.bvh_ready) {
        std::vector<d4> sph64;
        for (uint32_t prim : slots) {
            if (prim < ns) {
                const RayzSphere& q = s->spheres[prim];
                sph64.push_back(d4{q.center[0], q.center[1], q.center[2], q.radius * q.radius});
                sph64.push_back(d4{q.velocity[0], q.velocity[1], q.velocity[2], 0.0});
            } else { // triangle slot: unused by the narrow phase
                sph64.push_back(d4{0, 0, 0, 0});
                sph64.push_back(d4{0, 0, 0, 0});
            }
        }
        HIP_TRY(s->narrow.bvh_sph64.upload(sph64));
        s->narrow.bvh_ready = true;
    }
    if (b.bvh_ready) return RAYZ_OK;
    b.bvh_leaf_stride = s->triangles.empty() ? 2u : 3u;
    // one record per INNER node holding its two children's boxes (narrowed outward to f32: never smaller than the f64
    // box) + in lo.w where each child leads: an inner index, or kBvhLeafFlag | leaf descriptor
    // (first << 4 | type1 << 3 | type0 << 2 | count)
    std::vector<u4> nodes;
    std::vector<r4> leaf;
    // the inner nodes the kernel keeps in LDS (the tree's "top") are numbered first, the rest in pre-order
    std::vector<uint32_t> inner_index(t.nodes.size(), 0xffffffffu), inner_order;
    uint32_t n_inner = 0;
    {
        // top-of-tree records kept in LDS: as many as fit beside the stacks of the one-path kernel's workgroup (the two-path
        // kernel, with its smaller workgroups, keeps a prefix of them); RAYZ_DEBUG_BVH_TOP lowers the cap
        const size_t stacks = bvh_stack_bytes(t.depth, kBvhWg) + (t.big.empty() ? 0 : kBvhBigLdsBytes); // (+ the oversized hittables' records)
        const size_t lds_for_top = stacks < kBvhLdsBudget ? kBvhLdsBudget - stacks : 0;
        // WHICH record format (DevScene::bvh_nodes): 16-bit plane indices halve the bytes a step fetches and double the
        // records the LDS top holds, for 12 conversions per step — worth it only when most steps fetch from global memory,
        // i.e. for a tree much larger than the f32 top (measured: profiles/r03/lds_top).  RAYZ_DEBUG_BVH_NODES forces one.
        size_t inner_total = 0;
        for (const rayz_bvh::FlatNode& n : t.nodes) inner_total += n.count == 0;
        const long long format = tuning(RAYZ_DEBUG_BVH_NODES, 0);
        b.quantized = format == 2 || (format == 0 && inner_total > kQuantizeAboveTops * (lds_for_top / 64));
        const uint32_t fit = (uint32_t)(lds_for_top / (b.quantized ? 32 : 64));
        const uint32_t top_cap = (uint32_t)std::min<long long>(tuning(RAYZ_DEBUG_BVH_TOP, fit), fit);
        // WHICH records: grown from the root, always taking the candidate whose box has the largest surface area next — the
        // chance that a ray visits a node goes with its box's area, and never exceeds its parent's (RAYZ_DEBUG_BVH_TOP_ORDER
        // = 1: plain breadth-first, the order of rounds 2-3a)
        auto area = [&](size_t i) {
            const rayz_bvh::Box& x = t.nodes[i].box;
            const double dx = x.hi[0] - x.lo[0], dy = x.hi[1] - x.lo[1], dz = x.hi[2] - x.lo[2];
            return dx * dy + dy * dz + dz * dx;
        };
        const bool by_area = tuning(RAYZ_DEBUG_BVH_TOP_ORDER, 0) == 0;
        typedef std::pair<double, size_t> Cand; // (priority, node): largest first; breadth-first = decreasing sequence numbers
        std::priority_queue<Cand> frontier;
        double seq = 0;
        if (!t.nodes.empty() && t.nodes[0].count == 0) frontier.push({by_area ? area(0) : seq--, 0});
        while (!frontier.empty() && n_inner < top_cap) {
            const size_t i = frontier.top().second;
            frontier.pop();
            inner_index[i] = n_inner++;
            inner_order.push_back((uint32_t)i);
            for (size_t c : {i + 1, (size_t)t.nodes[i + 1].skip})
                if (t.nodes[c].count == 0) frontier.push({by_area ? area(c) : seq--, c});
        }
        b.bvh_top = n_inner;
        for (size_t i = 0; i < t.nodes.size(); ++i)
            if (t.nodes[i].count == 0 && inner_index[i] == 0xffffffffu) {
                inner_index[i] = n_inner++;
                inner_order.push_back((uint32_t)i);
            }
    }
    // the boxes go to the device PADDED: the slab test carries no slack of its own (bvh_walk.hpp: bvh_box_hit;
    // E = 16u·max(S, B) for f32 planes rounded outward, 16u·(max(S, B) + X) for plane indices on a grid of extent X)
    double box_B = 0;
    rayz_bvh::Box all;
    for (const rayz_bvh::FlatNode& n : t.nodes) {
        all.enclose(n.box);
        for (int k = 0; k < 3; ++k) box_B = std::max({box_B, std::fabs(n.box.lo[k]), std::fabs(n.box.hi[k])});
    }
    if (t.nodes.empty())
        for (int k = 0; k < 3; ++k) all.lo[k] = all.hi[k] = 0;
    double box_pad = kBoxPadUlps * unit_roundoff<float>() * std::max(b.pad_S, box_B);
    b.grid = rayz_bvh::PlaneGrid{}; // origin 0, cell 1: a plane is its own index
    if (b.quantized) {
        box_pad = kBoxPadUlps * unit_roundoff<float>() * (std::max(b.pad_S, box_B) + 2.0 * box_B);
        b.grid = rayz_bvh::PlaneGrid::over(all.lo, all.hi, 2.0 * box_pad);
        box_pad = kBoxPadUlps * unit_roundoff<float>() * (std::max(b.pad_S, box_B) + b.grid.extent); // (extent <= 2 B + 4 pad: within the margin)
    }
    auto leaf_info = [&](const rayz_bvh::FlatNode& n) {
        uint32_t info = (n.first << 4) | n.count;
        for (uint32_t k = 0; k < n.count; ++k)
            if (t.order[n.first + k] >= ns) info |= 1u << (2 + k);
        return info;
    };
    auto fbits = [](float f) {
        uint32_t w;
        std::memcpy(&w, &f, 4);
        return w;
    };
    auto child = [&](size_t c) {
        const rayz_bvh::FlatNode& n = t.nodes[c];
        const bool is_leaf = n.count != 0;
        const uint32_t ref = is_leaf ? (kBvhLeafFlag | leaf_info(n)) : (inner_index[c] << (b.quantized ? 5 : 6)); // inner: byte offset
        if (b.quantized) {
            uint32_t w[3];
            b.grid.quantize(n.box, box_pad, w);
            nodes.push_back(u4{w[0], w[1], w[2], ref});
        } else {
            nodes.push_back(u4{fbits(rayz_bvh::roundDown<float>(n.box.lo[0] - box_pad)), fbits(rayz_bvh::roundDown<float>(n.box.lo[1] - box_pad)),
                               fbits(rayz_bvh::roundDown<float>(n.box.lo[2] - box_pad)), ref});
            nodes.push_back(u4{fbits(rayz_bvh::roundUp<float>(n.box.hi[0] + box_pad)), fbits(rayz_bvh::roundUp<float>(n.box.hi[1] + box_pad)),
                               fbits(rayz_bvh::roundUp<float>(n.box.hi[2] + box_pad)), 0u});
        }
    };
    if (!t.nodes.empty() && t.nodes[0].count != 0) { // the whole pool fits one leaf: a root record whose two child
        child(0);                                     // slots both name it (the repeat cannot change the result)
        child(0);
        n_inner = 1;
    } else {
        for (uint32_t i : inner_order) { // records in index order
            child((size_t)i + 1);             // left child follows its parent in pre-order
            child(t.nodes[i + 1].skip);       // right child = where the left subtree ends
        }
    }
    if (n_inner >= (1u << 25)) // the walk addresses a record by a 32-bit byte offset (index << 6)
        return fail(RAYZ_ERR_BAD_ARG, "BVH of %u inner nodes exceeds the device layout (2^25)", n_inner);
    b.bvh_n_inner = t.nodes.empty() ? 0u : n_inner;
    for (uint32_t prim : slots) {
        if (prim < ns) {
            const RayzSphere& q = s->spheres[prim];
            leaf.push_back(r4{(R)q.center[0], (R)q.center[1], (R)q.center[2], (R)pad_radius2_scan<R>(q, b.pad_S)});
            leaf.push_back(r4{(R)q.velocity[0], (R)q.velocity[1], (R)q.velocity[2], Bits<R>::from(prim)});
            if (b.bvh_leaf_stride == 3) leaf.push_back(r4{R(0), R(0), R(0), R(0)});
        } else {
            const RayzTriangle& q = s->triangles[prim - ns];
            leaf.push_back(r4{(R)q.v0[0], (R)q.v0[1], (R)q.v0[2], Bits<R>::from(prim)});
            leaf.push_back(r4{(R)(q.v1[0] - q.v0[0]), (R)(q.v1[1] - q.v0[1]), (R)(q.v1[2] - q.v0[2]), R(0)});
            leaf.push_back(r4{(R)(q.v2[0] - q.v0[0]), (R)(q.v2[1] - q.v0[1]), (R)(q.v2[2] - q.v0[2]), R(0)});
        }
    }
    HIP_TRY(b.bvh_nodes.upload(nodes));
    HIP_TRY(b.bvh_leaf.upload(leaf));
    b.bvh_ready = true;
    return RAYZ_OK;
}

template <class R> int upload_bvh(RayzScene* s, SceneBuffers<R>& b) {
    if (b.bvh_ready && s->narrow.bvh_ready) return RAYZ_OK;
    const int rc = upload_bvh_body<R>(s, b);
    if (rc != RAYZ_OK) { // drop the partly built BVH buffers (the scan streams stay valid)
        b.bvh_nodes.reset();
        b.bvh_leaf.reset();
        b.bvh_ready = false;
        if (!s->narrow.bvh_ready) s->narrow.bvh_sph64.reset();
    }
    return rc;
}

// Nesting depth of every texture (solid = 1, checker = 1 + deeper child); 0 marks a cycle.  The device walks a
// checker chain with a bounded loop (kMaxTextureDepth lookups) where the reference recurses without a limit
// (src/material.zig:36-37): a pool the loop cannot resolve is refused here instead of rendering black.
int texture_depths(const RayzSceneDesc* d, std::vector<uint32_t>& depth) {
    const uint32_t n = d->n_textures;
    depth.assign(n, 0u);
    std::vector<uint8_t> state(n, 0); // 0 unvisited, 1 on the stack, 2 done
    std::vector<uint32_t> stack;
    for (uint32_t root = 0; root < n; ++root) {
        if (state[root]) continue;
        stack.push_back(root);
        while (!stack.empty()) {
            const uint32_t i = stack.back();
            const RayzTexture& t = d->textures[i];
            if (t.kind == RAYZ_TEX_SOLID) {
                depth[i] = 1, state[i] = 2;
                stack.pop_back();
                continue;
            }
            if (state[i] == 0) {
                state[i] = 1;
                bool pushed = false;
                for (uint32_t c : {t.even, t.odd}) {
                    if (state[c] == 1) return fail(RAYZ_ERR_BAD_ARG, "texture %u: checker chain contains a cycle (through %u)", i, c);
                    if (state[c] == 0) stack.push_back(c), pushed = true;
                }
                if (pushed) continue;
            }
            // both children done (or were done already)
            if (state[t.even] != 2 || state[t.odd] != 2) { // a child is still on the stack below us: a cycle
                return fail(RAYZ_ERR_BAD_ARG, "texture %u: checker chain contains a cycle", i);
            }
            depth[i] = 1 + (depth[t.even] > depth[t.odd] ? depth[t.even] : depth[t.odd]);
            state[i] = 2;
            stack.pop_back();
        }
    }
    return RAYZ_OK;
}

int validate_scene(const RayzSceneDesc* d) {
    if (!d) return fail(RAYZ_ERR_BAD_ARG, "scene is null");
    if ((d->n_spheres && !d->spheres) || (d->n_materials && !d->materials) || (d->n_textures && !d->textures) ||
        (d->n_triangles && !d->triangles))
        return fail(RAYZ_ERR_BAD_ARG, "scene list pointer is null");
    for (uint32_t i = 0; i < d->n_triangles; ++i)
        if (d->triangles[i].material >= d->n_materials)
            return fail(RAYZ_ERR_BAD_ARG, "triangle %u: material handle %u out of range", i, d->triangles[i].material);
    for (uint32_t i = 0; i < d->n_textures; ++i) {
        const RayzTexture& t = d->textures[i];
        if (t.kind > RAYZ_TEX_SOLID) return fail(RAYZ_ERR_BAD_ARG, "texture %u: bad kind %u", i, t.kind);
        if (t.kind == RAYZ_TEX_CHECKER && (t.even >= d->n_textures || t.odd >= d->n_textures))
            return fail(RAYZ_ERR_BAD_ARG, "texture %u: checker handle out of range", i);
    }
    {
        std::vector<uint32_t> depth;
        RAYZ_TRY(texture_depths(d, depth));
        for (uint32_t i = 0; i < d->n_textures; ++i)
            if (depth[i] > (uint32_t)kMaxTextureDepth)
                return fail(RAYZ_ERR_BAD_ARG, "texture %u: checker nesting depth %u exceeds the device limit %d", i, depth[i],
                            kMaxTextureDepth);
    }
    for (uint32_t i = 0; i < d->n_materials; ++i) {
        const RayzMaterial& m = d->materials[i];
        if (m.kind > RAYZ_MAT_DIELECTRIC) return fail(RAYZ_ERR_BAD_ARG, "material %u: bad kind %u", i, m.kind);
        if (m.kind != RAYZ_MAT_DIELECTRIC && m.texture >= d->n_textures)
            return fail(RAYZ_ERR_BAD_ARG, "material %u: texture handle %u out of range", i, m.texture);
        if (m.kind == RAYZ_MAT_DIFFUSE && m.method > RAYZ_DIFFUSE_HEMISPHERE)
            return fail(RAYZ_ERR_BAD_ARG, "material %u: bad diffuse method %u", i, m.method);
    }
    for (uint32_t i = 0; i < d->n_spheres; ++i)
        if (d->spheres[i].material >= d->n_materials)
            return fail(RAYZ_ERR_BAD_ARG, "sphere %u: material handle %u out of range", i, d->spheres[i].material);
    return RAYZ_OK;
}

int validate_params(const RayzRenderParams* p) {
    if (!p) return fail(RAYZ_ERR_BAD_ARG, "params is null");
    if (!p->width || !p->height || !p->samples_per_px) return fail(RAYZ_ERR_BAD_ARG, "width, height and samples_per_px must be > 0");
    if (p->precision > RAYZ_PRECISION_F64) return fail(RAYZ_ERR_BAD_ARG, "bad precision %u", p->precision);
    if (p->traversal > RAYZ_TRAVERSAL_AUTO) return fail(RAYZ_ERR_BAD_ARG, "bad traversal %u", p->traversal);
    const uint32_t sc = p->shard_count ? p->shard_count : 1;
    if (p->shard_index >= sc) return fail(RAYZ_ERR_BAD_ARG, "shard_index %u >= shard_count %u", p->shard_index, sc);
    if (!(p->tmin == p->tmin)) return fail(RAYZ_ERR_BAD_ARG, "tmin is NaN");
    if (chunk_count(p) >= kMaxChunksPerPx) // whatever chunk_spp is, 0 (the automatic schedule) included
        return fail(RAYZ_ERR_BAD_ARG, "more than 2^20 chunks per pixel (%llu): raise chunk_spp", (unsigned long long)chunk_count(p));
    return RAYZ_OK;
}

template <class R> void fill_camera(const RayzCameraDesc* c, DevCamera<R>& o) {
    for (int k = 0; k < 3; ++k) {
        o.from[k] = (R)c->look_from[k];
        o.du[k] = (R)c->px_du[k];
        o.dv[k] = (R)c->px_dv[k];
        o.pxo[k] = (R)c->px_origin[k];
        o.defu[k] = (R)c->defocus_u[k];
        o.defv[k] = (R)c->defocus_v[k];
    }
    o.defocus = c->defocus ? 1u : 0u;
    o._pad = 0;
}

// ---- device contexts -----------------------------------------------------------------------------------
int ensure_ctx(int device) { // creates the context of `device` if needed; g_mu held by the caller (ensure_ctx_locked: taken here)
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(RAYZ_ERR_NO_DEVICE, "no HIP device: %s", hipGetErrorString(e));
    if (device < 0 || device >= n || device >= RAYZ_MAX_DEVICES)
        return fail(RAYZ_ERR_BAD_ARG, "device %d out of range [0,%d)", device, n < RAYZ_MAX_DEVICES ? n : RAYZ_MAX_DEVICES);
    DeviceCtx& c = g_ctx[device];
    if (c.ok) return RAYZ_OK;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RAYZ_ERR_NO_DEVICE, "device %d is %s; this library carries gfx950 code only", device, prop.gcnArchName);
    DeviceScope scope(device);
    HIP_TRY(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    c.num_cu = prop.multiProcessorCount;
    c.ok = true;
    return RAYZ_OK;
}


int ensure_ctx_locked(int device) {
    std::lock_guard<std::mutex> lock(g_mu);
    return ensure_ctx(device);
}

// The scene's device side for a render of `p` with `cam`: the buffers uploaded (their filter padded for the camera's origin
// bound) and, when the render walks the BVH, the tree.  A scene supports ONE render in flight: a launch on another stream first
// waits for the previous one (its workspace and counters are reused, and a re-upload frees buffers it may still read).
// (ray queries pass their own origin bound `S`: the largest |origin| of the batch, rayz_hip_scene_query)
template <class R>
int prepare_scene_bound(RayzScene* s, SceneBuffers<R>& b, double S, uint32_t traversal, hipStream_t stream, bool& use_bvh) {
    use_bvh = traversal == RAYZ_TRAVERSAL_BVH ||
              (traversal == RAYZ_TRAVERSAL_AUTO && s->spheres.size() + s->triangles.size() > RAYZ_AUTO_BVH_MIN);
    if (s->spheres.size() + s->triangles.size() >= (1u << 27))
        return fail(RAYZ_ERR_BAD_ARG, "too many hittables for the device layout");
    if (s->last_stream && s->last_stream != stream) HIP_TRY(hipStreamSynchronize(s->last_stream)); // previous render done
    if (s->origin_bound < 0) s->origin_bound = scene_origin_bound(s);
    RAYZ_TRY(upload<R>(s, b, std::max(s->origin_bound, S)));
    if (use_bvh) {
        RAYZ_TRY(upload_bvh<R>(s, b));
        if (s->bvh_dev.depth > (uint32_t)kBvhStackDepth)
            return fail(RAYZ_ERR_BAD_ARG, "BVH depth %u exceeds the traversal stack (%d)", s->bvh_dev.depth, kBvhStackDepth);
    }
    return RAYZ_OK;
}

template <class R>
int prepare_scene(RayzScene* s, SceneBuffers<R>& b, const RayzCameraDesc* cam, const RayzRenderParams* p, hipStream_t stream,
                  bool& use_bvh) {
    return prepare_scene_bound<R>(s, b, camera_origin_bound(cam), p->traversal, stream, use_bvh);
}

// Work items of a launch over `chunks` chunks of a shard of `shard_pixels` pixels: the queue head, its reservations and the
// place_item arithmetic are u32.
int check_items(uint64_t shard_pixels, uint64_t chunks) {
    const uint64_t items = shard_pixels * chunks;
    if (shard_pixels >= (1ull << 31) || items >= (1ull << 32) - (1ull << 26))
        return fail(RAYZ_ERR_BAD_ARG, "too many work items (%llu): raise chunk_spp", (unsigned long long)items);
    return RAYZ_OK;
}

// What a trace launch runs.  trace_window fills it for the product kernels; with a BVH, experiment_override may then swap in a
// retired kernel with its own workgroup and LDS needs.
template <class R> struct BvhLaunchPlan {
    void (*kernel)(const TraceArgs<R>);
    int block;               // threads per workgroup
    size_t stack_bytes;      // LDS: the per-lane traversal stacks, after the tree's top
    size_t extra_lds_bytes;  // LDS: behind the oversized hittables' records (no product kernel has any)
    uint32_t top_records;    // records of the tree's top the workgroup keeps in LDS, at most
    uint32_t items_per_lane; // work items a lane holds at a time (sizes the grid)
    int experiment;          // 0: a product kernel; else which retired kernel (scene_sync reports by it)
};

// The retired experiment kernels' host side (trace_kernel_bvh2: two paths per lane; trace_kernel_bvhx: walker / shader waves —
// DESIGN.md §6): only a -DRAYZ_EXPERIMENTS build contains it.  The product build has these hooks instead: nothing to override or
// report, and the refusals of the retired kernels' knobs.
#ifdef RAYZ_EXPERIMENTS
#include "experiments/launch.hpp"
#else
template <class R> int experiment_override(BvhLaunchPlan<R>&, TraceArgs<R>&, const RayzScene*, const SceneBuffers<R>&, const RayzRenderParams*) { return RAYZ_OK; }
template <class R> void experiment_lds_placed(TraceArgs<R>&, uint32_t) {}
inline int experiment_sync(int, const unsigned long long*) { return RAYZ_OK; }
inline int experiment_knob_check(uint32_t knob, long long value) {
    if (knob == RAYZ_DEBUG_BVH_KERNEL) {
        if (value != 1) return fail(RAYZ_ERR_BAD_ARG, "BVH_KERNEL %lld: this build holds the one-path kernel only (the retired two-path "
                                                      "experiment needs -DRAYZ_EXPERIMENTS)", value);
        return RAYZ_OK;
    }
    if (knob == RAYZ_DEBUG_BVH2_KEEP) return fail(RAYZ_ERR_BAD_ARG, "BVH2_KEEP: the two-path kernel is not in this build (-DRAYZ_EXPERIMENTS)");
    return fail(RAYZ_ERR_BAD_ARG, "BVHX: the exchange kernel is not in this build (-DRAYZ_EXPERIMENTS)");
}
#endif

// The LDS request of a launch: `top_records` records of the tree's top (rec_bytes each) in front of `fixed_bytes` (stacks |
// oversized hittables' records | ..).  The top was sized for kBvhLdsBudget, which this driver stack accepts; should a stack refuse
// the request (hipFuncSetAttribute fails, or the occupancy query finds room for no workgroup), the launch keeps a SHORTER PREFIX
// of the top instead of failing every BVH launch — the walk works with any prefix (records beyond it are read from global
// memory), only slower.  Returns with the prefix kept in top_records, the bytes to ask for in `lds` and the workgroups a CU holds.
// (A kernel without dynamic LDS, fixed_bytes = 0 and no top, passes with whatever the occupancy query says.)
template <class K>
int request_lds(K kernel, const char* what, int block, size_t rec_bytes, size_t fixed_bytes, uint32_t& top_records, size_t& lds, int& blocks_per_cu) {
    for (;;) {
        lds = (size_t)top_records * rec_bytes + fixed_bytes;
        hipError_t e = hipSuccess;
        if (lds > 64 * 1024) // a workgroup that asks for more than 64 KB of LDS has to say so first
            e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e == hipSuccess) e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, kernel, block, lds);
        if (e == hipSuccess && (blocks_per_cu >= 1 || lds == 0)) return RAYZ_OK;
        (void)hipGetLastError(); // (clear the sticky error of the refused request)
        if (top_records == 0)
            return fail(RAYZ_ERR_HIP, "the %s kernel cannot be launched with %zu bytes of LDS: %s", what, lds,
                        e == hipSuccess ? "no workgroup fits a CU" : hipGetErrorString(e));
        const uint32_t step = (uint32_t)(8192 / rec_bytes); // give back 8 KB of the top per try
        top_records = top_records > step ? top_records - step : 0u;
    }
}

// The dynamic LDS of a BVH kernel's workgroup: top | stacks | oversized hittables' records | `extra_bytes` of the caller's own.
// `stack_bytes` is a parameter, not a depth, because a retired kernel gives stacks to some of its waves only.
struct BvhLds {
    uint32_t top_records = 0; // records of the tree's top the workgroup keeps: what was asked for, or a prefix of it (request_lds)
    size_t lds = 0;           // bytes to launch with
    int blocks_per_cu = 0;    // workgroups a CU holds with that
    uint32_t top_bytes = 0;   // DevScene::bvh_top (the walk compares byte offsets)
    uint32_t top_words = 0, big_words = 0, extra_words = 0; // where the stacks, the oversized records and the extra bytes start (u32s)
};
template <class K>
int bvh_lds_layout(K kernel, const char* what, int block, size_t stack_bytes, bool quantized, uint32_t n_big_leaves,
                   uint32_t top_records, size_t extra_bytes, BvhLds& L) {
    const size_t big_bytes = n_big_leaves ? kBvhBigLdsBytes : 0, rec_bytes = quantized ? 32 : 64;
    L.top_records = top_records;
    RAYZ_TRY(request_lds(kernel, what, block, rec_bytes, stack_bytes + big_bytes + extra_bytes, L.top_records, L.lds, L.blocks_per_cu));
    const size_t top_bytes = (size_t)L.top_records * rec_bytes;
    L.top_bytes = (uint32_t)top_bytes;
    L.top_words = (uint32_t)(top_bytes / sizeof(uint32_t));
    L.big_words = (uint32_t)((top_bytes + stack_bytes) / sizeof(uint32_t));
    L.extra_words = (uint32_t)((top_bytes + stack_bytes + big_bytes) / sizeof(uint32_t));
    return RAYZ_OK;
}

// The scene as a kernel sees it: the buffers of precision R and the shared narrow-phase buffers.  bvh_top stays 0: bytes of the tree's
// top in LDS, which the launch sets once it knows how many records its workgroup keeps (bvh_lds_layout).
template <class R> DevScene<R> dev_scene(const RayzScene& s, const SceneBuffers<R>& b, bool use_bvh) {
    DevScene<R> sc{};
    sc.stat = b.stat, sc.movy = b.movy, sc.movg = b.movg;
    sc.slot64 = s.narrow.slot64, sc.slot_pool = s.narrow.slot_pool;
    sc.sph_pool = b.sph_pool, sc.mat = b.mat, sc.tex = b.tex;
    sc.ns_pad = s.narrow.ns_pad, sc.ny_pad = s.narrow.ny_pad, sc.ng_pad = s.narrow.ng_pad;
    sc.n_spheres = (uint32_t)s.spheres.size();
    sc.tri = b.tri, sc.nt_pad = b.nt_pad, sc.n_triangles = (uint32_t)s.triangles.size();
    sc.bvh_nodes = (const f4*)b.bvh_nodes.get();
    for (int k = 0; k < 3; ++k) sc.bvh_glo[k] = b.grid.glo[k], sc.bvh_cell[k] = b.grid.cell[k];
    sc.bvh_leaf = b.bvh_leaf, sc.bvh_leaf_stride = b.bvh_leaf_stride, sc.bvh_sph64 = s.narrow.bvh_sph64;
    sc.bvh_n_nodes = use_bvh ? b.bvh_n_inner : 0u;
    sc.bvh_n_big_leaves = use_bvh ? b.n_big_leaves : 0u;
    for (int k = 0; k < 4; ++k) sc.bvh_big[k] = b.big_desc[k];
    sc.bvh_top = 0u;
    return sc;
}

// A shard of `p`'s frame (rows dealt in interleaved tiles of tile_rows rows): the two defaulted parameters, the shard's rows and
// how many of its pixels lie in whole 8x8 tiles of those local rows (place_item).
struct ShardGeometry { uint32_t tile_rows, shard_count, rows, tiled_pixels; };
ShardGeometry shard_geometry(const RayzRenderParams* p) {
    ShardGeometry g{p->tile_rows ? p->tile_rows : RAYZ_DEFAULT_TILE_ROWS, p->shard_count ? p->shard_count : 1u, 0u, 0u};
    for (uint32_t t = p->shard_index; p->shard_index < g.shard_count && (uint64_t)t * g.tile_rows < p->height; t += g.shard_count) {
        const uint32_t r0 = t * g.tile_rows;
        g.rows += (p->height - r0 < g.tile_rows) ? p->height - r0 : g.tile_rows;
    }
    g.tiled_pixels = p->width % 8 == 0 ? (uint32_t)((uint64_t)(g.rows / 8 * 8) * p->width) : 0u;
    return g;
}

// One launch of the trace kernel over the chunk WINDOW [c0, c1) of `p`'s shard (prepare_scene done, the device selected):
// queue entry k · shard_pixels + i sums the samples of chunk c0 + k of the i-th pixel into the scene's workspace, partial[k ·
// shard_pixels + local pixel] (grown here to the window).  `d_starts` is the device copy of the WHOLE schedule `starts`;
// p->samples_per_px stays the total, so every sample keeps its stream (pixel · spp + s): a chunk's sum does not depend on the
// window it is traced in.  The first `reset_bytes` of `counters` are cleared first (the queue head, counters[0], at least);
// ev0 / ev1 bracket the kernel; `experiment` returns BvhLaunchPlan::experiment.
// With `active_list` (an adaptive pass): the window's chunks of the list's `n_active` pixels only, through the
// adaptive_pass_kernel[_bvh] — queue entry k · n_active + j sums chunk c0 + k of pixel active_list[j] into partial[k · n_active + j].
// The cells kernel of a scan form.  Defined at the very end of this file, and named nowhere else: the compiler emits
// a kernel where it first meets a reference to it, so these come out behind every other kernel, and the labels it numbers through the
// whole file (a long branch's) keep their numbers in every kernel from before — tests/test_sparse_isa.py holds those kernels' text
// label for label.
void (*cells_kernel_f32(uint32_t form))(const CellsTraceArgs<float>);
void (*cells_kernel_f64(uint32_t form))(const CellsTraceArgs<double>);
template <class R> auto cells_kernel(uint32_t form) {
    if constexpr (sizeof(R) == 8) return cells_kernel_f64(form);
    else return cells_kernel_f32(form);
}

template <class R>
int trace_window(RayzScene* s, const DeviceCtx& ctx, SceneBuffers<R>& b, const RayzCameraDesc* cam, const RayzRenderParams* p,
                 bool use_bvh, const std::vector<uint32_t>& starts, const uint32_t* d_starts, uint32_t c0, uint32_t c1,
                 unsigned long long* counters, size_t reset_bytes, hipEvent_t ev0, hipEvent_t ev1, hipStream_t stream,
                 int& experiment, const uint32_t* active_list = nullptr, uint32_t n_active = 0, PrimaryLists* lists = nullptr) {
    typedef typename VecOf<R>::type r4;
    const ShardGeometry shard = shard_geometry(p);
    const uint64_t shard_pixels64 = (uint64_t)shard.rows * p->width;
    const uint32_t chunks_per_px = c1 - c0;
    const uint64_t traced_pixels64 = active_list ? n_active : shard_pixels64;
    const uint64_t items64 = traced_pixels64 * chunks_per_px;
    RAYZ_TRY(check_items(shard_pixels64, 1));
    RAYZ_TRY(check_items(traced_pixels64, chunks_per_px));
    const size_t need = (size_t)items64 * sizeof(r4);
    if (need > s->partial.capacity()) {
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(s->partial.grow(need));
    }

    TraceArgs<R> A{};
    A.sc = dev_scene<R>(*s, b, use_bvh);
    fill_camera<R>(cam, A.cam);
    A.partial = (r4*)s->partial.get();
    A.counters = counters;
    A.seed = p->seed;
    A.tmin = (R)p->tmin;
    A.width = p->width;
    A.height = p->height;
    A.spp = p->samples_per_px;
    A.max_bounces = p->max_bounces;
    A.chunk_start = d_starts + c0; // (chunk_bounds indexes the table with the window's own k)
    A.chunks_per_px = chunks_per_px;
    A.chunk_uniform = starts[1]; // the table's uniform prefix (chunk_bounds): chunks of starts[1] samples while the table keeps that stride
    A.chunk_n_uniform = 0;
    // .. computed from the WINDOW's k, which is the chunk's own index only in a window that starts at chunk 0: later windows read
    // every chunk's bounds from the table (tools/progressive_bench.py measures what that costs)
    while (c0 == 0 && A.chunk_n_uniform < chunks_per_px && starts[A.chunk_n_uniform + 1] == (A.chunk_n_uniform + 1) * A.chunk_uniform) A.chunk_n_uniform++;
    A.tile_rows = shard.tile_rows;
    A.shard_index = p->shard_index;
    A.shard_count = shard.shard_count;
    A.shard_pixels = (uint32_t)shard_pixels64;
    A.tiled_pixels = shard.tiled_pixels;
    A.total_items = (uint32_t)items64;
    A.queue_grab = (uint32_t)std::max(1ll, tuning(RAYZ_DEBUG_QUEUE_GRAB, kQueueGrab));
    A.n_active = active_list ? n_active : 0u;
    A.active_list = active_list;
    // scheduling thresholds of the BVH kernel (no effect on results; rayz_hip_debug_set refuses values outside 1 .. 64 lanes)
    A.bvh_keep = (uint32_t)tuning(RAYZ_DEBUG_BVH_KEEP, kBvhKeepActive | (kBvhKeepStepping << 8));

    BvhLaunchPlan<R> plan{};
    plan.kernel = active_list ? adaptive_pass_kernel<R, 1> : trace_kernel<R, 1>;
    // the xy basis where the scene's layout prices it lower (or the caller asked for it): the same candidates' narrow phase, the same image
    if (!active_list && !use_bvh && scene_scan_form(s) == rayz_plane::kScanFormXY) plan.kernel = flat_xy_kernel<R, 1>;
    // .. and the kernel that scans the one-radius sets in their own two-field loop: the XY basis, the same candidates and more
    if (!active_list && !use_bvh && scene_scan_form(s) == rayz_plane::kScanFormOneRadius) plan.kernel = flat_one_radius_kernel<R, 1>;
    // .. and each of the three with the camera segments from the pixels' primary lists, where the scene takes them (`lists`: the
    // caller's, built below inside the launch's events unless they hold this camera's already)
    const bool primary = lists && !active_list && !use_bvh && scene_primary_lists(s, p->samples_per_px);
    if (primary) {
        const size_t words = (size_t)(rayz_primary::kListK + 1u) * (size_t)shard_pixels64;
        if (words > lists->buf.capacity()) {
            HIP_TRY(hipStreamSynchronize(stream));
            HIP_TRY(lists->buf.alloc(words));
            lists->built = false;
        }
    }
    plan.block = 256;
    plan.items_per_lane = 1;
    if (use_bvh) {
        if (active_list) plan.kernel = b.quantized ? adaptive_pass_kernel_bvh<R, true> : adaptive_pass_kernel_bvh<R, false>;
        else plan.kernel = b.quantized ? trace_kernel_bvh<R, true> : trace_kernel_bvh<R, false>;
        plan.block = (int)kBvhWg;
        plan.stack_bytes = bvh_stack_bytes(s->bvh_dev.depth, kBvhWg);
        // the tree's top: first in LDS.  The scene numbered b.bvh_top records breadth-first for this kernel's workgroup
        plan.top_records = b.bvh_top;
        if (!active_list) RAYZ_TRY(experiment_override<R>(plan, A, s, b, p)); // (the product build: nothing; no retired kernel reads a list)
    }
    experiment = plan.experiment;
    // The LDS request (+ RAYZ_DEBUG_LDS_PAD unused bytes behind the kernel's own: an occupancy experiment — fewer workgroups per CU,
    // the same code).  The flat list's kernel has no dynamic LDS: no stacks, no top, nothing extra.
    const size_t extra_bytes = use_bvh ? plan.extra_lds_bytes + (size_t)tuning(RAYZ_DEBUG_LDS_PAD, 0) : 0;
    BvhLds L;
    RAYZ_TRY(bvh_lds_layout(plan.kernel, "trace", plan.block, plan.stack_bytes, b.quantized, use_bvh ? b.n_big_leaves : 0u, plan.top_records,
                            extra_bytes, L));
    A.bvh_top_words = L.top_words;
    A.bvh_big_words = L.big_words;
    A.sc.bvh_top = L.top_bytes;
    experiment_lds_placed<R>(A, L.extra_words);
    uint64_t grid = (uint64_t)ctx.num_cu * std::max(1, L.blocks_per_cu);
    const uint64_t per_block = (uint64_t)plan.items_per_lane * plan.block;
    const uint64_t want = (items64 + per_block - 1) / per_block;
    if (grid > want) grid = want;

    HIP_TRY(hipMemsetAsync(counters, 0, reset_bytes, stream));
    HIP_TRY(hipEventRecord(ev0, stream));
    if (primary && !lists->built) {
        PrimaryArgs B{};
        for (int k = 0; k < 3; ++k) {
            B.cam.from[k] = cam->look_from[k], B.cam.du[k] = cam->px_du[k], B.cam.dv[k] = cam->px_dv[k];
            B.cam.pxo[k] = cam->px_origin[k], B.cam.defu[k] = cam->defocus_u[k], B.cam.defv[k] = cam->defocus_v[k];
        }
        B.cam.defocus = cam->defocus ? 1u : 0u;
        B.slot64 = s->narrow.slot64, B.real_slots = s->narrow.real_slots, B.lists = lists->buf;
        B.n_real = s->narrow.n_real;
        B.width = p->width, B.tile_rows = shard.tile_rows, B.shard_index = p->shard_index, B.shard_count = shard.shard_count;
        B.shard_pixels = A.shard_pixels;
        hipLaunchKernelGGL(primary_lists_kernel, dim3((uint32_t)((shard_pixels64 + 255) / 256)), dim3(256), 0, stream, B);
        HIP_TRY(hipGetLastError());
        lists->built = true;
    }
    // .. and each of the three with every listable segment from the slab's cells (and the primary lists, if the launch has them):
    // one-shot and progressive renders alone (`lists` names them), and only with a positive tmin — the query keeps the ray's t >= 0
    if (lists && !active_list && !use_bvh && p->tmin > 0.0 && scene_cell_lists(s)) {
        CellsTraceArgs<R> P{};
        static_cast<TraceArgs<R>&>(P) = A;
        const uint32_t* built_lists = lists->buf;
        P.primary = primary ? built_lists : nullptr;
        P.grid = s->narrow.cell_grid;
        P.cells = s->narrow.cell_table;
        // AUTO walks only from kWalkMinMembers members on (a smaller pool's scan is cheaper than a walk); a forced ON always walks
        if (!(s->cells_mode == RAYZ_CELL_LISTS_ON || s->narrow.cell_members >= rayz_cells::kWalkMinMembers)) P.grid.any_overflowed |= rayz_cells::kNoWalk;
#ifdef RAYZ_CELLS_TUNE // measurement builds only: the thresholds from the environment
        P.grid.list_lanes = std::getenv("RAYZ_CELLS_LIST_LANES") ? (uint32_t)std::atoi(std::getenv("RAYZ_CELLS_LIST_LANES")) : rayz_cells::kListLanes;
        P.grid.max_cells = std::getenv("RAYZ_CELLS_MAX_CELLS") ? (uint32_t)std::atoi(std::getenv("RAYZ_CELLS_MAX_CELLS")) : rayz_cells::kMaxCells;
        P.grid.walk_columns = rayz_cells::kWalkColumns;
        if (std::getenv("RAYZ_CELLS_WALK_COLUMNS")) // (a cap named here overrides AUTO's gate too)
            P.grid.walk_columns = (uint32_t)std::atoi(std::getenv("RAYZ_CELLS_WALK_COLUMNS")), P.grid.any_overflowed &= ~rayz_cells::kNoWalk;
        P.grid.one_class = std::getenv("RAYZ_CELLS_ONE_CLASS") ? (uint32_t)std::atoi(std::getenv("RAYZ_CELLS_ONE_CLASS")) : 0u;
#endif
        const uint32_t form = scene_scan_form(s);
        void (*kernel)(const CellsTraceArgs<R>) = cells_kernel<R>(form);
        static int occupancy[4] = {0, 0, 0, 0}; // by scan form, of precision R; 0: not asked yet
        int& blocks_per_cu = occupancy[form & 3u];
        if (blocks_per_cu == 0) HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, kernel, plan.block, 0));
        grid = std::min<uint64_t>((uint64_t)ctx.num_cu * std::max(1, blocks_per_cu), want);
        hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(plan.block), 0, stream, P);
    } else if (primary) { // the same launch geometry (the flat kernels have no dynamic LDS), the lists behind the arguments
        PrimaryTraceArgs<R> P{};
        static_cast<TraceArgs<R>&>(P) = A;
        P.primary = lists->buf;
        const uint32_t form = scene_scan_form(s);
        void (*kernel)(const PrimaryTraceArgs<R>) = form == rayz_plane::kScanFormOneRadius ? primary_one_radius_kernel<R, 1>
                                                    : form == rayz_plane::kScanFormXY      ? primary_xy_kernel<R, 1>
                                                                                           : primary_xz_kernel<R, 1>;
        // its own occupancy (the persistent grid is one resident wave set of THIS kernel), asked for once per kernel
        static int occupancy[4] = {0, 0, 0, 0}; // by scan form, of precision R; 0: not asked yet
        int& blocks_per_cu = occupancy[form & 3u];
        if (blocks_per_cu == 0) HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks_per_cu, kernel, plan.block, 0));
        grid = std::min<uint64_t>((uint64_t)ctx.num_cu * std::max(1, blocks_per_cu), want);
        hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(plan.block), 0, stream, P);
    } else {
        hipLaunchKernelGGL(plan.kernel, dim3((uint32_t)grid), dim3(plan.block), L.lds, stream, A);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev1, stream));
    return RAYZ_OK;
}

// The device copy of the schedule `starts` (scene->chunk_start), kept until the schedule changes.
int scene_schedule(RayzScene* s, const std::vector<uint32_t>& starts, hipStream_t stream) {
    if (starts == s->chunk_start_host) return RAYZ_OK;
    HIP_TRY(hipStreamSynchronize(stream));
    HIP_TRY(s->chunk_start.grow(starts.size()));
    HIP_TRY(hipMemcpy(s->chunk_start, starts.data(), starts.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    s->chunk_start_host = starts;
    return RAYZ_OK;
}

// Launches one render of `p`'s shard on the scene's device: the trace kernel over every chunk, then resolve_kernel.  The caller
// has selected that device (DeviceScope).
template <class R>
int render_impl(RayzScene* s, const DeviceCtx& ctx, SceneBuffers<R>& b, const RayzCameraDesc* cam, const RayzRenderParams* p,
                R* d_out, hipStream_t stream) {
    typedef typename VecOf<R>::type r4;
    bool use_bvh = false;
    RAYZ_TRY(prepare_scene<R>(s, b, cam, p, stream, use_bvh));

    const uint32_t rows = rayz_hip_shard_rows(p);
    const uint64_t shard_pixels64 = (uint64_t)rows * p->width;
    std::vector<uint32_t> starts;
    chunk_schedule(p, starts);
    const uint32_t chunks_per_px = (uint32_t)starts.size() - 1;
    const uint64_t items64 = shard_pixels64 * chunks_per_px;
    RAYZ_TRY(check_items(shard_pixels64, chunks_per_px));
    s->last = RayzRenderStats{};
    s->last.primary_rays = shard_pixels64 * p->samples_per_px;
    s->last_bvh = use_bvh;
    s->last_experiment = 0;
    s->last_sparse = false;
    if (items64 == 0) {
        s->rendered = false;
        return RAYZ_OK;
    }
    if (!d_out) return fail(RAYZ_ERR_BAD_ARG, "output pointer is null");
    s->last_stream = stream;
    if (p->max_bounces == 0) { // bounceRay(ray, 0) is black, src/renderer.zig:104-105
        HIP_TRY(hipMemsetAsync(d_out, 0, shard_pixels64 * 3 * sizeof(R), stream));
        s->rendered = false;
        return RAYZ_OK;
    }
    if (!s->counters) HIP_TRY(s->counters.alloc(32));
    RAYZ_TRY(scene_schedule(s, starts, stream));
    if (!s->ev0) {
        HIP_TRY(s->ev0.create());
        HIP_TRY(s->ev1.create());
    }
    s->primary.built = false; // (no cache across renders: this camera's lists are built by this launch)
    RAYZ_TRY(trace_window<R>(s, ctx, b, cam, p, use_bvh, starts, s->chunk_start, 0, chunks_per_px, s->counters,
                             32 * sizeof(unsigned long long), s->ev0, s->ev1, stream, s->last_experiment, nullptr, 0, &s->primary));
    hipLaunchKernelGGL(resolve_kernel<R>, dim3((uint32_t)((shard_pixels64 + 255) / 256)), dim3(256), 0, stream,
                       (const r4*)s->partial.get(), d_out, (uint32_t)shard_pixels64, chunks_per_px, p->samples_per_px);
    HIP_TRY(hipGetLastError());
    s->rendered = true;
    return RAYZ_OK;
}

int check_render_args(RayzScene* s, const RayzCameraDesc* cam, const RayzRenderParams* p, uint32_t precision) {
    if (!s) return fail(RAYZ_ERR_STATE, "scene handle is null");
    if (!cam) return fail(RAYZ_ERR_BAD_ARG, "camera is null");
    RAYZ_TRY(validate_params(p));
    if (p->precision != precision)
        return fail(RAYZ_ERR_BAD_ARG, "params.precision %u does not match this entry point", p->precision);
    return RAYZ_OK;
}

template <class R>
int render_device(RayzScene* s, const RayzCameraDesc* cam, const RayzRenderParams* p, R* d_out, void* stream_arg, uint32_t precision) {
    RAYZ_TRY(check_render_args(s, cam, p, precision));
    DeviceCtx* ctx = nullptr;
    hipStream_t stream = nullptr;
    RAYZ_TRY(scene_stream(s->device, stream_arg, ctx, stream));
    DeviceScope scope(s->device);
    return render_impl<R>(s, *ctx, buffers_of<R>(*s), cam, p, d_out, stream);
}

// (a handle is built in a unique_ptr and released to the caller at the end: an exception on the way, which guarded() reports,
// takes the half-built handle with it)
int scene_new(const RayzSceneDesc* scene, int device, std::unique_ptr<RayzScene>& out) {
    RAYZ_TRY(validate_scene(scene));
    auto s = std::make_unique<RayzScene>();
    s->spheres.assign(scene->spheres, scene->spheres + scene->n_spheres);
    s->materials.assign(scene->materials, scene->materials + scene->n_materials);
    s->textures.assign(scene->textures, scene->textures + scene->n_textures);
    s->triangles.assign(scene->triangles, scene->triangles + scene->n_triangles);
    s->device = device;
    out = std::move(s);
    return RAYZ_OK;
}

int scene_create(const RayzSceneDesc* scene, int device, RayzScene** out) {
    if (!out) return fail(RAYZ_ERR_BAD_ARG, "out handle pointer is null");
    *out = nullptr;
    std::unique_ptr<RayzScene> s;
    const int rc = scene_new(scene, device, s);
    *out = s.release();
    return rc;
}

// The 32 counters of a finished launch, read back into `st`: the segments the kernel counted (`own_segments`; a query's are its rays,
// in `st` already), the sphere tests — counted by a BVH walk, every hittable of `s` per segment for the flat list — and the BVH's
// node tests.  A BVH kernel's refusal to run (`kernel`: its name) is the launch's failure.  `inspect` sees the raw counters first.
template <class F>
int read_counters(const RayzScene& s, const unsigned long long* d_counters, const char* kernel, bool bvh, bool own_segments,
                  RayzRenderStats& st, F&& inspect) {
    unsigned long long c[32] = {};
    HIP_TRY(hipMemcpy(c, d_counters, sizeof(c), hipMemcpyDeviceToHost));
    RAYZ_TRY(inspect(c));
    if (bvh && c[31]) return fail(RAYZ_ERR_STATE, "%s refused to run: its dynamic LDS segment does not start at LDS address 0", kernel);
    if (own_segments) st.segments = c[1];
    st.sphere_tests = bvh ? c[3] : st.segments * (unsigned long long)(s.spheres.size() + s.triangles.size());
    st.node_tests = bvh ? c[2] : 0;
    return RAYZ_OK;
}
int nothing_to_inspect(const unsigned long long*) { return RAYZ_OK; }

int scene_sync(RayzScene* s, RayzRenderStats* stats) {
    if (!s) return fail(RAYZ_ERR_STATE, "scene handle is null");
    if (s->device < 0) { // never rendered: nothing to wait for
        if (stats) *stats = s->last;
        return RAYZ_OK;
    }
    DeviceScope scope(s->device);
    if (s->last_stream) HIP_TRY(hipStreamSynchronize(s->last_stream));
    if (s->rendered) {
        auto report = [&](const unsigned long long* c) { // (measurement builds: the phase profile of the kernel that ran)
#ifdef RAYZ_FLAT_PROFILE // measurement build only: wave time per phase of trace_kernel
        if (!s->last_bvh && c[9]) {
            const double tot = (double)(c[4] + c[5] + c[6] + c[7] + c[8] + c[10]);
            std::fprintf(stderr, "flat phases (share of wave time; ticks per wave-iteration %.0f): refill %.1f%% | setup %.1f%% | scan %.1f%% | "
                                 "flush %.1f%% | shade %.1f%% | list phases %.1f%%; ticks: scans+flush %.4g, list %.4g, all %.4g; scans %llu\n",
                         tot / (double)c[9], 100.0 * c[4] / tot, 100.0 * c[5] / tot, 100.0 * c[6] / tot, 100.0 * c[7] / tot, 100.0 * c[8] / tot,
                         100.0 * c[10] / tot, (double)(c[6] + c[7]), (double)c[10], tot, c[9]);
            if (c[11]) { // a cells kernel ran (trace_kernel_flat.hpp: fp)
                std::fprintf(stderr, "cells: secondary segments %llu, listable by the box %.2f%%, by the walk %.2f%%; cell-lane segments listed %llu (%.2f entries each); list phases %llu "
                                     "(%.1f lanes each); live lanes per scan %.1f; cells per listable secondary segment:",
                             c[11], 100.0 * c[12] / (double)c[11], 100.0 * c[18] / (double)c[11], c[13], (double)c[14] / (double)(c[13] ? c[13] : 1), c[15],
                             (double)c[16] / (double)(c[15] ? c[15] : 1), (double)c[17] / (double)(c[9] ? c[9] : 1));
#ifdef RAYZ_FLAT_PROFILE_WALK // (trace_kernel_flat.hpp: the slots hold the walk's histogram instead)
                static const char* const bins[8] = {"<= 4", "<= 8", "<= 12", "<= 16", "<= 24", "<= 32", "<= 48", "more"};
                unsigned long long all = 0;
                for (int k = 0; k < 8; ++k) all += c[19 + k] & ((1ull << 30) - 1ull);
                std::fprintf(stderr, " (not in this build)\nwalk: secondary segments whose box fails on its count alone %llu (%.2f%%); by columns, share and walk cells each:",
                             all, 100.0 * (double)all / (double)c[11]);
                for (int k = 0; k < 8; ++k) {
                    const unsigned long long n = c[19 + k] & ((1ull << 30) - 1ull), cells = c[19 + k] >> 30;
                    std::fprintf(stderr, " %s: %.2f%% %.1f |", bins[k], 100.0 * (double)n / (double)(all ? all : 1), (double)cells / (double)(n ? n : 1));
                }
#else
                for (int k = 0; k <= 12; ++k) std::fprintf(stderr, " %d: %.2f%%", k, 100.0 * c[19 + k] / (double)(c[12] ? c[12] : 1));
#endif
                std::fprintf(stderr, "\n");
            }
        }
#endif
#ifdef RAYZ_BVH_PROFILE // measurement build only: per-phase wave time and lane occupancy of the BVH kernel
        if (s->last_bvh && !s->last_experiment) {
            const double tot = (double)(c[4] + c[5] + c[6] + c[7] + c[8]);
            std::fprintf(stderr,
                         "bvh phases (share of wave time | mean active lanes): refill %.1f%% | N %.1f%% %.1f | L %.1f%% %.1f | C %.1f%% "
                         "%.1f | shade %.1f%% %.1f\n",
                         100.0 * c[4] / tot, 100.0 * c[5] / tot, (double)c[9] / (double)(c[10] ? c[10] : 1), 100.0 * c[6] / tot,
                         (double)c[11] / (double)(c[12] ? c[12] : 1), 100.0 * c[7] / tot, (double)c[13] / (double)(c[14] ? c[14] : 1),
                         100.0 * c[8] / tot, (double)c[1] / (double)(c[15] ? c[15] : 1));
            const double it = (double)(c[10] ? c[10] : 1);
            std::fprintf(stderr, "  box steps: lanes per wave-step — stepping %.1f | parked at a leaf %.1f | walk finished, waiting for the shading pass %.1f | "
                                 "no path %.1f; wave-steps per segment %.2f; shading passes %.3g, rounds %.3g\n",
                         (double)c[9] / it, (double)c[16] / it, (double)c[17] / it, (double)c[18] / it, it / (double)(c[1] ? c[1] : 1) * 1.0,
                         (double)c[15], (double)c[12]);
            std::fprintf(stderr, "  node fetch (issue -> data): %.1f%% of the box-step phase, %.0f ticks per wave-step\n",
                         100.0 * (double)c[19] / (double)(c[5] ? c[5] : 1), (double)c[19] / it);
        }
#endif
            // a retired kernel ran: its phase profile (measurement builds) and its abort flag
            return s->last_experiment ? experiment_sync(s->last_experiment, c) : (int)RAYZ_OK;
        };
        RayzRenderStats st = s->last;
        RAYZ_TRY(read_counters(*s, s->counters, "trace_kernel_bvh", s->last_bvh, true, st, report));
        float ms = 0;
        if (s->last_sparse) HIP_TRY(hipEventElapsedTime(&ms, s->sparse_ev[0], s->sparse_ev[1])); // (the call's check, trace and resolve)
        else HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
        st.kernel_ms = ms;
        s->last = st;
    }
    if (stats) *stats = s->last;
    return RAYZ_OK;
}

int scene_free(RayzScene* s) {
    delete s; // (~RayzScene waits for the scene's last launch)
    return RAYZ_OK;
}

template <class R>
int render_oneshot(const RayzSceneDesc* scene, const RayzCameraDesc* cam, const RayzRenderParams* p, R* out,
                   RayzRenderStats* stats, uint32_t precision) {
    if (!out) return fail(RAYZ_ERR_BAD_ARG, "output pointer is null");
    RAYZ_TRY(validate_params(p));
    int device = default_device_or_none();
    if (device < 0) {
        RAYZ_TRY(rayz_hip_init(0));
        device = 0;
    }
    std::unique_ptr<RayzScene> s;
    RAYZ_TRY(scene_new(scene, device, s));
    DeviceScope scope(device);
    const size_t n = (size_t)rayz_hip_shard_rows(p) * p->width * 3;
    DevBuf<R> d_out; // (declared after the scene: freed first, as ever)
    hipError_t e = d_out.alloc(n);
    if (e != hipSuccess) return fail(RAYZ_ERR_OOM, "hipMalloc(output): %s", hipGetErrorString(e));
    int rc = render_device<R>(s.get(), cam, p, d_out.get(), nullptr, precision);
    if (rc == RAYZ_OK) rc = scene_sync(s.get(), stats);
    if (rc == RAYZ_OK && n) {
        e = hipMemcpy(out, d_out, n * sizeof(R), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(RAYZ_ERR_HIP, "hipMemcpy(output): %s", hipGetErrorString(e));
    }
    return rc;
}

} // namespace

extern "C" {

uint32_t rayz_hip_abi_version(void) { return RAYZ_HIP_ABI_VERSION; }

int rayz_hip_debug_set(uint32_t knob, long long value) {
    if (knob >= RAYZ_DEBUG_KNOBS) return fail(RAYZ_ERR_BAD_ARG, "bad debug knob %u", knob);
    // A knob changes scheduling, never a result — and must never be able to hang the device: values a kernel's loop
    // control cannot take are refused here (negative = back to the built-in default, always accepted).
    if (value >= 0) {
        auto lane_count = [](long long b) { return b >= 1 && b <= 64; }; // a threshold counted in lanes of a wave
        switch (knob) {
        case RAYZ_DEBUG_QUEUE_GRAB:
            if (value < 1 || value > (1 << 20)) return fail(RAYZ_ERR_BAD_ARG, "QUEUE_GRAB %lld outside 1 .. 2^20", value);
            break;
        case RAYZ_DEBUG_BVH_KEEP: // keep_active | keep_stepping << 8
            if (value >> 16 || !lane_count(value & 0xff) || !lane_count((value >> 8) & 0xff))
                return fail(RAYZ_ERR_BAD_ARG, "BVH_KEEP 0x%llx: both thresholds must be 1 .. 64 lanes", (unsigned long long)value);
            break;
        case RAYZ_DEBUG_BVH_KERNEL:
        case RAYZ_DEBUG_BVH2_KEEP:
        case RAYZ_DEBUG_BVHX: // the retired kernels' knobs: checked in experiments/launch.hpp, refused by the product build
            RAYZ_TRY(experiment_knob_check(knob, value));
            break;
        case RAYZ_DEBUG_CHUNK_CAP:
#ifdef RAYZ_EXPERIMENTS
            if (value < 16 || value > 4096 || (value & (value - 1))) return fail(RAYZ_ERR_BAD_ARG, "CHUNK_CAP %lld: a power of two, 16 .. 4096", value);
#else
            return fail(RAYZ_ERR_BAD_ARG, "CHUNK_CAP changes the image's summation tree: -DRAYZ_EXPERIMENTS builds only");
#endif
            break;
        case RAYZ_DEBUG_DENOISE_LDS_STRIDE:
            if (value != 0 && value != 1 && value != 2 && value != 4) return fail(RAYZ_ERR_BAD_ARG, "DENOISE_LDS_STRIDE %lld: 0 (no level staged), 1, 2 or 4", value);
            break;
        case RAYZ_DEBUG_LDS_PAD:
            if (value > 160 * 1024) return fail(RAYZ_ERR_BAD_ARG, "LDS_PAD %lld exceeds a CU's LDS", value);
            break;
        default: break;
        }
    }
    g_tune.v[knob].store(value, std::memory_order_relaxed);
    return RAYZ_OK;
}
const char* rayz_hip_last_error(void) { return g_err; }

int rayz_hip_init(int device) {
    return guarded([&] {
        std::lock_guard<std::mutex> lock(g_mu);
        const int rc = ensure_ctx(device);
        if (rc == RAYZ_OK) g_default = device;
        return rc;
    });
}

void rayz_hip_shutdown(void) {
    std::lock_guard<std::mutex> lock(g_mu);
    for (int d = 0; d < RAYZ_MAX_DEVICES; ++d) {
        DeviceCtx& c = g_ctx[d];
        if (!c.ok) continue;
        DeviceScope scope(d);
        (void)hipStreamSynchronize(c.stream);
        (void)hipStreamDestroy(c.stream);
        c = DeviceCtx{};
    }
    g_default = -1;
}

uint32_t rayz_hip_shard_rows(const RayzRenderParams* p) { return p ? shard_geometry(p).rows : 0; }

uint32_t rayz_hip_chunk_schedule(const RayzRenderParams* p, uint32_t* starts, uint32_t capacity) {
    if (!p || !p->samples_per_px || !p->width || !p->height) return 0;
    if (chunk_count(p) >= kMaxChunksPerPx) return 0; // a schedule no render accepts (validate_params)
    std::vector<uint32_t> v;
    try {
        chunk_schedule(p, v);
    } catch (...) {
        return 0;
    }
    if (v.size() - 1 != chunk_count(p)) return 0; // chunk_count is exact by construction: a disagreement is a bug, not a schedule
    if (starts)
        for (size_t i = 0; i < v.size() && i < capacity; ++i) starts[i] = v[i];
    return (uint32_t)v.size() - 1;
}

int rayz_hip_scene_create(const RayzSceneDesc* scene, RayzScene** out) {
    return guarded([&] { return scene_create(scene, -1, out); });
}

int rayz_hip_scene_create_on(int device, const RayzSceneDesc* scene, RayzScene** out) {
    return guarded([&] {
        if (out) *out = nullptr;
        RAYZ_TRY(ensure_ctx_locked(device));
        return scene_create(scene, device, out);
    });
}

int rayz_hip_scene_destroy(RayzScene* s) {
    return guarded([&] { return scene_free(s); });
}

int rayz_hip_render_device(RayzScene* s, const RayzCameraDesc* cam, const RayzRenderParams* p, float* d_out,
                           void* stream) {
    return guarded([&] { return render_device<float>(s, cam, p, d_out, stream, RAYZ_PRECISION_F32); });
}

int rayz_hip_render_device_f64(RayzScene* s, const RayzCameraDesc* cam, const RayzRenderParams* p, double* d_out,
                               void* stream) {
    return guarded([&] { return render_device<double>(s, cam, p, d_out, stream, RAYZ_PRECISION_F64); });
}

int rayz_hip_scene_set_scan_form(RayzScene* s, uint32_t form) {
    return guarded([&] {
        if (!s) return fail(RAYZ_ERR_BAD_ARG, "null scene");
        if (form > RAYZ_SCAN_FORM_ONE_RADIUS) return fail(RAYZ_ERR_BAD_ARG, "bad scan form %u", form);
        s->scan_form = form;
        return (int)RAYZ_OK;
    });
}

int rayz_hip_scene_get_scan_form(RayzScene* s, uint32_t* form) {
    return guarded([&] {
        if (!s || !form) return fail(RAYZ_ERR_BAD_ARG, "null argument");
        *form = scene_scan_form(s);
        return (int)RAYZ_OK;
    });
}

int rayz_hip_scene_set_primary_lists(RayzScene* s, uint32_t mode) {
    return guarded([&] {
        if (!s) return fail(RAYZ_ERR_BAD_ARG, "null scene");
        if (mode > RAYZ_PRIMARY_LISTS_ON) return fail(RAYZ_ERR_BAD_ARG, "bad primary-lists mode %u", mode);
        s->primary_mode = mode;
        return (int)RAYZ_OK;
    });
}

int rayz_hip_scene_get_primary_lists(RayzScene* s, uint32_t samples_per_px, uint32_t* on) {
    return guarded([&] {
        if (!s || !on) return fail(RAYZ_ERR_BAD_ARG, "null argument");
        *on = scene_primary_lists(s, samples_per_px) ? 1u : 0u;
        return (int)RAYZ_OK;
    });
}

int rayz_hip_scene_set_cell_lists(RayzScene* s, uint32_t mode) {
    return guarded([&] {
        if (!s) return fail(RAYZ_ERR_BAD_ARG, "null scene");
        if (mode > RAYZ_CELL_LISTS_ON) return fail(RAYZ_ERR_BAD_ARG, "bad cell-lists mode %u", mode);
        s->cells_mode = mode;
        return (int)RAYZ_OK;
    });
}

int rayz_hip_scene_get_cell_lists(RayzScene* s, uint32_t* on) {
    return guarded([&] {
        if (!s || !on) return fail(RAYZ_ERR_BAD_ARG, "null argument");
        *on = scene_cell_lists(s) ? 1u : 0u;
        return (int)RAYZ_OK;
    });
}

int rayz_hip_scene_sync(RayzScene* s, RayzRenderStats* stats) {
    return guarded([&] { return scene_sync(s, stats); });
}

int rayz_hip_scene_bvh(RayzScene* s, uint32_t* n_nodes, uint32_t* depth, double* boxes, uint32_t* skip, uint32_t* first,
                       uint32_t* count, uint32_t* order) {
    return guarded([&] {
        if (!s || !n_nodes) return fail(RAYZ_ERR_BAD_ARG, "null argument");
        ensure_bvh(s);
        const rayz_bvh::FlatBvh& t = s->bvh;
        *n_nodes = (uint32_t)t.nodes.size();
        if (depth) *depth = t.depth;
        for (size_t i = 0; i < t.nodes.size(); ++i) {
            if (boxes)
                for (int k = 0; k < 3; ++k) boxes[6 * i + k] = t.nodes[i].box.lo[k], boxes[6 * i + 3 + k] = t.nodes[i].box.hi[k];
            if (skip) skip[i] = t.nodes[i].skip;
            if (first) first[i] = t.nodes[i].first;
            if (count) count[i] = t.nodes[i].count;
        }
        if (order) std::copy(t.order.begin(), t.order.end(), order);
        return (int)RAYZ_OK;
    });
}

int rayz_hip_render(const RayzSceneDesc* scene, const RayzCameraDesc* cam, const RayzRenderParams* p, float* out,
                    RayzRenderStats* stats) {
    return guarded([&] { return render_oneshot<float>(scene, cam, p, out, stats, RAYZ_PRECISION_F32); });
}

int rayz_hip_render_f64(const RayzSceneDesc* scene, const RayzCameraDesc* cam, const RayzRenderParams* p, double* out,
                        RayzRenderStats* stats) {
    return guarded([&] { return render_oneshot<double>(scene, cam, p, out, stats, RAYZ_PRECISION_F64); });
}

int rayz_hip_tonemap_u8(const float* d_rgb, uint8_t* d_rgb8, size_t n_pixels, void* stream) {
    return guarded([&] {
        int device;
        hipStream_t own;
        RAYZ_TRY(default_device(device, own));
        if (!n_pixels) return (int)RAYZ_OK;
        if (!d_rgb || !d_rgb8) return fail(RAYZ_ERR_BAD_ARG, "null buffer");
        DeviceScope scope(device);
        const size_t n = n_pixels * 3;
        hipLaunchKernelGGL(tonemap_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream_or(stream, own), d_rgb, d_rgb8, n);
        HIP_TRY(hipGetLastError());
        return (int)RAYZ_OK;
    });
}

} // extern "C"

// ---- the features on top of the trace launch (order: see the head of this file) ---------------------------------------------
#include "progressive.hpp"
#include "adaptive_passes.hpp"
#include "sparse_render.hpp"
#include "known_answers.hpp"
#include "multi_device.hpp"
#include "query.hpp"
#include "chain.hpp"
#include "sampled.hpp"
#include "frame_handle.hpp"
#include "denoiser.hpp"
#include "upscaler.hpp"
#include "temporal.hpp"
#include "temporal_moments.hpp"

// ---- the cells kernels, named last (see cells_kernel) ----
namespace {
template <class R> void (*cells_kernel_of(uint32_t form))(const CellsTraceArgs<R>) {
    using namespace rayz_dev_cells;
    return form == rayz_plane::kScanFormOneRadius ? cells_one_radius_kernel<R, 1> : form == rayz_plane::kScanFormXY ? cells_xy_kernel<R, 1> : cells_xz_kernel<R, 1>;
}
void (*cells_kernel_f32(uint32_t form))(const CellsTraceArgs<float>) { return cells_kernel_of<float>(form); }
void (*cells_kernel_f64(uint32_t form))(const CellsTraceArgs<double>) { return cells_kernel_of<double>(form); }
} // namespace
