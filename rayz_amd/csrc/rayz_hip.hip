// rayz_hip.hip — the C ABI of include/rayz_hip.h: scene upload, workspace, kernel launches.
//
// Replaces the body of `Tracer.render()` (src/renderer.zig:72-101 of jlucier/rayz).  A scene handle is bound to
// ONE device (its own context: stream, CU count); a process may drive several devices — one scene per device,
// rows dealt in interleaved tiles (params.shard_*) — either itself (rayz_hip_multi_*: one host thread, one stream
// per device, one RCCL gather of the row tiles to the first device) or as one process per GPU with the gather
// done by the caller (torch.distributed in bench.py).
#include "../../include/rayz_hip.h"
#include "rayz_device.hpp"
#include "bvh_build.hpp"
#include "denoise.hpp"
#include "noise.hpp"

#include <rccl/rccl.h> // types and prototypes only: the library is opened with dlopen at the first multi-device call

#include <dlfcn.h>

#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <limits>
#include <mutex>
#include <algorithm>
#include <atomic>
#include <new>
#include <queue>
#include <memory>
#include <type_traits>
#include <utility>
#include <vector>

using namespace rayz_dev;

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// No exception crosses the C ABI: every extern "C" body that can allocate runs inside guarded().
template <class F> int guarded(F&& f) noexcept {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return fail(RAYZ_ERR_OOM, "host allocation failed");
    } catch (const std::exception& e) {
        return fail(RAYZ_ERR_HIP, "unexpected exception: %s", e.what());
    } catch (...) {
        return fail(RAYZ_ERR_HIP, "unexpected exception");
    }
}

// One context per HIP device ordinal, created by rayz_hip_init(device) (or lazily by the *_on / multi entries).
struct DeviceCtx {
    bool ok = false;
    hipStream_t stream = nullptr;
    int num_cu = 0;
};
DeviceCtx g_ctx[RAYZ_MAX_DEVICES];

// Measurement knobs (rayz_hip_debug_set; they change scheduling or the walked tree, never an image).  The library reads
// no environment variable: a stray one cannot change a production render.  -1 = the built-in default.
struct Tuning {
    std::atomic<long long> v[RAYZ_DEBUG_KNOBS];
    Tuning() { for (auto& x : v) x.store(-1, std::memory_order_relaxed); }
};
Tuning g_tune; // written by rayz_hip_debug_set, read (once per knob) by the render / scene build that starts next
long long tuning(int knob, long long dflt) {
    const long long x = g_tune.v[knob].load(std::memory_order_relaxed);
    return x < 0 ? dflt : x;
}
int g_default = -1; // device of the last successful rayz_hip_init: what entry points without a device argument use
std::mutex g_mu;    // guards g_ctx / g_default

// HIP's current device is per host thread: every entry point that touches a device selects it and restores the
// caller's on return (the host may be torch, with its own idea of the current device).
struct DeviceScope {
    int prev = -1, dev;
    explicit DeviceScope(int d) : dev(d) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceScope() {
        if (prev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

// The owners of everything this file allocates on a device.  Both are move-only and remember the HIP ordinal that was current
// when they allocated: reset() and the destructor free with that device selected, whatever the calling thread's is.
// DevBuf<T>: one hipMalloc allocation of capacity() elements (DevBuf<char>: bytes).
template <class T> class DevBuf {
    T* p_ = nullptr;
    size_t cap_ = 0;
    int dev_ = -1;

public:
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept { *this = std::move(o); }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            reset();
            p_ = std::exchange(o.p_, nullptr), cap_ = std::exchange(o.cap_, 0), dev_ = o.dev_;
        }
        return *this;
    }
    ~DevBuf() { reset(); }
    void reset() {
        if (!p_) return;
        DeviceScope scope(dev_);
        (void)hipFree(p_);
        p_ = nullptr, cap_ = 0;
    }
    hipError_t alloc(size_t n) { // (no elements: 16 bytes all the same, so that get() is a pointer a kernel may be handed)
        reset();
        hipError_t e = hipGetDevice(&dev_);
        if (e == hipSuccess) e = hipMalloc((void**)&p_, n ? n * sizeof(T) : 16);
        if (e == hipSuccess) cap_ = n;
        else p_ = nullptr;
        return e;
    }
    hipError_t upload(const std::vector<T>& v) {
        const hipError_t e = alloc(v.size());
        return e == hipSuccess && !v.empty() ? hipMemcpy(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice) : e;
    }
    // Grow-only: frees first, so the caller has waited for whatever may still use the old allocation.
    hipError_t grow(size_t n) { return p_ && n <= cap_ ? hipSuccess : alloc(n); }
    size_t capacity() const { return cap_; }
    T* get() const { return p_; }
    operator T*() const { return p_; }
};
typedef DevBuf<char> DevBytes;

class DevEvent {
    hipEvent_t ev_ = nullptr;
    int dev_ = -1;

public:
    DevEvent() = default;
    DevEvent(DevEvent&& o) noexcept { *this = std::move(o); }
    DevEvent& operator=(DevEvent&& o) noexcept {
        if (this != &o) {
            reset();
            ev_ = std::exchange(o.ev_, nullptr), dev_ = o.dev_;
        }
        return *this;
    }
    ~DevEvent() { reset(); }
    void reset() {
        if (!ev_) return;
        DeviceScope scope(dev_);
        (void)hipEventDestroy(ev_);
        ev_ = nullptr;
    }
    hipError_t create(unsigned flags = hipEventDefault) {
        reset();
        hipError_t e = hipGetDevice(&dev_);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&ev_, flags);
        if (e != hipSuccess) ev_ = nullptr;
        return e;
    }
    operator hipEvent_t() const { return ev_; }
};

#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return fail(e_ == hipErrorOutOfMemory ? RAYZ_ERR_OOM : RAYZ_ERR_HIP, "%s: %s (%s:%d)", #expr,     \
                        hipGetErrorString(e_), __FILE__, __LINE__);                                         \
    } while (0)

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
    DevBuf<d4> bvh_sph64; // leaf order (BVH traversal only)
    uint32_t ns_pad = 0, ny_pad = 0, ng_pad = 0;
    // slot order of the static (0) and mov-Y (1) classes: plane runs first (rayz_plane::plan_runs), then the loose spheres
    std::vector<PlaneRun> runs[2];
    std::vector<std::vector<uint32_t>> run_members[2]; // pool indices of each run
    std::vector<uint32_t> loose[2];
    uint32_t plane_slots[2] = {0, 0};
    bool ready = false, bvh_ready = false;
};

uint32_t round_up(uint32_t v, uint32_t m) { return (v + m - 1) / m * m; }

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
    RayzRenderStats last{};
    // ray queries (rayz_hip_scene_query*): their own counters and events, so that rayz_hip_scene_sync keeps reporting the last render
    DevBuf<unsigned long long> q_counters; // [0] batch head, [2] node tests, [3] sphere tests, [31] LDS flag,
                                           // [kQueryBoundBase + k·kQueryBoundStride] the bound check's four words
    DevEvent q_ev0, q_ev1;
    hipStream_t q_stream = nullptr;
    bool queried = false, q_bvh = false;
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

int upload_narrow_body(RayzScene* s) {
    NarrowBuffers& nb = s->narrow;
    classify(s);
    // slot numbering is shared by both precisions: pad to the larger (f32) group size.  Static and mov-Y: plane runs,
    // each padded to whole group pairs, then the loose spheres
    static_assert(kStaticGroup == kMovYGroup, "one run padding for both classes");
    for (int c = 0; c < 2; ++c)
        nb.plane_slots[c] = rayz_plane::plan_runs(s->cls[c], [&](uint32_t pool) { return (float)s->spheres[pool].center[1]; },
                                                  kStaticGroup, nb.runs[c], nb.run_members[c], nb.loose[c]);
    nb.ns_pad = nb.plane_slots[0] + scan_len(nb.loose[0].size(), kStaticGroup);
    nb.ny_pad = nb.plane_slots[1] + scan_len(nb.loose[1].size(), kMovYGroup);
    nb.ng_pad = scan_len(s->cls[2].size(), kMovGGroup);
    const size_t slots = (size_t)nb.ns_pad + nb.ny_pad + nb.ng_pad;
    std::vector<d4> slot64(2 * slots, d4{0, 0, 0, 0});
    std::vector<uint32_t> slot_pool(slots, 0u);
    auto place = [&](size_t slot, uint32_t pool) {
        const RayzSphere& q = s->spheres[pool];
        slot64[2 * slot] = d4{q.center[0], q.center[1], q.center[2], q.radius * q.radius}; // radius * radius in f64, src/geom.zig:45
        slot64[2 * slot + 1] = d4{q.velocity[0], q.velocity[1], q.velocity[2], 0.0};
        slot_pool[slot] = pool;
    };
    const size_t class0[2] = {0, nb.ns_pad};
    for (int c = 0; c < 2; ++c) { // a run's members fill its first slots; its pads keep slot_pool 0 (never a candidate: r² = -inf)
        for (size_t j = 0; j < nb.runs[c].size(); ++j)
            for (size_t k = 0; k < nb.run_members[c][j].size(); ++k) place(class0[c] + nb.runs[c][j].first + k, nb.run_members[c][j][k]);
        for (size_t k = 0; k < nb.loose[c].size(); ++k) place(class0[c] + nb.plane_slots[c] + k, nb.loose[c][k]);
    }
    for (size_t k = 0; k < s->cls[2].size(); ++k) place((size_t)nb.ns_pad + nb.ny_pad + k, s->cls[2][k]);
    HIP_TRY(nb.slot64.upload(slot64));
    HIP_TRY(nb.slot_pool.upload(slot_pool));
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
    int rc = upload_narrow(s);
    if (rc != RAYZ_OK) return rc;
    auto rec = [&](uint32_t pool) { // w = the PADDED r² of the conservative filter
        const RayzSphere& q = s->spheres[pool];
        return r4{(R)q.center[0], (R)q.center[1], (R)q.center[2], (R)pad_radius2_scan<R>(q, b.pad_S)};
    };
    // static / mov-Y streams (f32 for both precisions): blocks of G spheres, SoA inside a block (field f of sphere k of
    // block g at g·W·G + f·G + k).  After the head (kPlaneHeader words: layout and run table, rayz_device.hpp), the plane
    // section — its runs at their slots, W = F − 1 fields (no cy: the run table holds it), two spare groups — then the
    // loose section, W = F, two spare groups.  Pad spheres {0, (0,) 0, r² = -inf, vy = 0}.
    const float ninf32 = -std::numeric_limits<float>::infinity();
    auto rec32 = [&](uint32_t pool) { // w = the PADDED r² of the conservative filter
        const RayzSphere& q = s->spheres[pool];
        return f4{(float)q.center[0], (float)q.center[1], (float)q.center[2], pad_radius2_scan<R>(q, b.pad_S)};
    };
    auto blocks = [&](int c, uint32_t F, uint32_t class_slots) {
        const NarrowBuffers& nb = s->narrow;
        const uint32_t G = group_size<float>(), P = F - 1;
        const uint32_t n_plane = nb.plane_slots[c] + 2 * G, n_loose = class_slots - nb.plane_slots[c] + 2 * G;
        std::vector<float> v(kPlaneHeader + (size_t)n_plane * P + (size_t)n_loose * F, 0.0f);
        const uint32_t head[4] = {(uint32_t)nb.runs[c].size(), nb.plane_slots[c], 0u, 0u}; // the stream's head (rayz_device.hpp)
        std::memcpy(v.data(), head, sizeof(head));
        std::memcpy(v.data() + 4, nb.runs[c].data(), nb.runs[c].size() * sizeof(PlaneRun));
        float* const plane = v.data() + kPlaneHeader;
        float* const loose = plane + (size_t)n_plane * P;
        for (uint32_t k = 0; k < n_plane; ++k) plane[(size_t)(k / G) * P * G + 2 * G + k % G] = ninf32;
        for (uint32_t k = 0; k < n_loose; ++k) loose[(size_t)(k / G) * F * G + 3 * G + k % G] = ninf32;
        for (size_t j = 0; j < nb.runs[c].size(); ++j)
            for (size_t m = 0; m < nb.run_members[c][j].size(); ++m) {
                const uint32_t pool = nb.run_members[c][j][m], k = nb.runs[c][j].first + (uint32_t)m;
                const f4 r = rec32(pool);
                float* blk = plane + (size_t)(k / G) * P * G + k % G;
                blk[0] = r.x, blk[G] = r.z, blk[2 * G] = r.w;
                if (F == 5) blk[3 * G] = (float)s->spheres[pool].velocity[1];
            }
        for (size_t k = 0; k < nb.loose[c].size(); ++k) {
            const uint32_t pool = nb.loose[c][k];
            const f4 r = rec32(pool);
            float* blk = loose + (k / G) * F * G + k % G;
            blk[0] = r.x, blk[G] = r.y, blk[2 * G] = r.z, blk[3 * G] = r.w;
            if (F == 5) blk[4 * G] = (float)s->spheres[pool].velocity[1];
        }
        return v;
    };
    const std::vector<float> stat = blocks(0, 4, s->narrow.ns_pad), movy = blocks(1, 5, s->narrow.ny_pad);
    std::vector<f4> movg(2 * (size_t)stream_len(s->cls[2].size(), kMovGGroup), f4{0.0f, 0.0f, 0.0f, 0.0f});
    for (size_t k = 0; k < movg.size(); k += 2) movg[k] = f4{0.0f, 0.0f, 0.0f, ninf32};
    for (size_t k = 0; k < s->cls[2].size(); ++k) {
        const RayzSphere& q = s->spheres[s->cls[2][k]];
        movg[2 * k] = rec32(s->cls[2][k]);
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
        const size_t stacks = ((size_t)t.depth + 3) * kBvhWg * sizeof(uint32_t) + (t.big.empty() ? 0 : kBvhBigLdsBytes); // (+ the oversized hittables' records)
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
    // the boxes go to the device PADDED: the slab test carries no slack of its own (rayz_device.hpp: bvh_box_hit;
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
        const int rc = texture_depths(d, depth);
        if (rc != RAYZ_OK) return rc;
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
int ensure_ctx(int device) { // creates the context of `device` if needed; g_mu held by the caller
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

// The context a scene renders on.  A scene created without a device is bound to the default device here.
int scene_ctx(RayzScene* s, DeviceCtx** out) {
    std::lock_guard<std::mutex> lock(g_mu);
    if (s->device < 0) {
        if (g_default < 0) return fail(RAYZ_ERR_NO_DEVICE, "rayz_hip_init has not succeeded");
        s->device = g_default;
    }
    if (!g_ctx[s->device].ok) return fail(RAYZ_ERR_NO_DEVICE, "device %d is not initialised (rayz_hip_init / shutdown order)", s->device);
    *out = &g_ctx[s->device];
    return RAYZ_OK;
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
    int rc = upload<R>(s, b, std::max(s->origin_bound, S));
    if (rc != RAYZ_OK) return rc;
    if (use_bvh) {
        rc = upload_bvh<R>(s, b);
        if (rc != RAYZ_OK) return rc;
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

// One launch of the trace kernel over the chunk WINDOW [c0, c1) of `p`'s shard (prepare_scene done, the device selected):
// queue entry k · shard_pixels + i sums the samples of chunk c0 + k of the i-th pixel into the scene's workspace, partial[k ·
// shard_pixels + local pixel] (grown here to the window).  `d_starts` is the device copy of the WHOLE schedule `starts`;
// p->samples_per_px stays the total, so every sample keeps its stream (pixel · spp + s): a chunk's sum does not depend on the
// window it is traced in.  The first `reset_bytes` of `counters` are cleared first (the queue head, counters[0], at least);
// ev0 / ev1 bracket the kernel; `experiment` returns BvhLaunchPlan::experiment.
template <class R>
int trace_window(RayzScene* s, const DeviceCtx& ctx, SceneBuffers<R>& b, const RayzCameraDesc* cam, const RayzRenderParams* p,
                 bool use_bvh, const std::vector<uint32_t>& starts, const uint32_t* d_starts, uint32_t c0, uint32_t c1,
                 unsigned long long* counters, size_t reset_bytes, hipEvent_t ev0, hipEvent_t ev1, hipStream_t stream,
                 int& experiment) {
    typedef typename VecOf<R>::type r4;
    const uint32_t rows = rayz_hip_shard_rows(p);
    const uint64_t shard_pixels64 = (uint64_t)rows * p->width;
    const uint32_t chunks_per_px = c1 - c0;
    const uint64_t items64 = shard_pixels64 * chunks_per_px;
    int rc = check_items(shard_pixels64, chunks_per_px);
    if (rc != RAYZ_OK) return rc;
    const size_t need = (size_t)items64 * sizeof(r4);
    if (need > s->partial.capacity()) {
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(s->partial.grow(need));
    }

    TraceArgs<R> A{};
    A.sc.stat = b.stat;
    A.sc.movy = b.movy;
    A.sc.movg = b.movg;
    A.sc.slot64 = s->narrow.slot64;
    A.sc.slot_pool = s->narrow.slot_pool;
    A.sc.sph_pool = b.sph_pool;
    A.sc.mat = b.mat;
    A.sc.tex = b.tex;
    A.sc.ns_pad = s->narrow.ns_pad;
    A.sc.ny_pad = s->narrow.ny_pad;
    A.sc.ng_pad = s->narrow.ng_pad;
    A.sc.n_spheres = (uint32_t)s->spheres.size();
    A.sc.tri = b.tri;
    A.sc.nt_pad = b.nt_pad;
    A.sc.n_triangles = (uint32_t)s->triangles.size();
    A.sc.bvh_nodes = (const f4*)b.bvh_nodes.get();
    for (int k = 0; k < 3; ++k) A.sc.bvh_glo[k] = b.grid.glo[k], A.sc.bvh_cell[k] = b.grid.cell[k];
    A.sc.bvh_leaf = b.bvh_leaf;
    A.sc.bvh_sph64 = s->narrow.bvh_sph64;
    A.sc.bvh_n_nodes = use_bvh ? b.bvh_n_inner : 0u;
    A.sc.bvh_leaf_stride = b.bvh_leaf_stride;
    A.sc.bvh_n_big_leaves = use_bvh ? b.n_big_leaves : 0u;
    for (int k = 0; k < 4; ++k) A.sc.bvh_big[k] = b.big_desc[k];
    A.sc.bvh_top = 0u; // (bytes: set below, once the launch knows how many records its workgroup keeps in LDS)
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
    A.tile_rows = p->tile_rows ? p->tile_rows : RAYZ_DEFAULT_TILE_ROWS;
    A.shard_index = p->shard_index;
    A.shard_count = p->shard_count ? p->shard_count : 1u;
    A.shard_pixels = (uint32_t)shard_pixels64;
    A.tiled_pixels = p->width % 8 == 0 ? (uint32_t)((uint64_t)(rows / 8 * 8) * p->width) : 0u; // whole 8x8 tiles of the local rows (place_item)
    A.total_items = (uint32_t)items64;
    A.queue_grab = (uint32_t)std::max(1ll, tuning(RAYZ_DEBUG_QUEUE_GRAB, kQueueGrab));
    // scheduling thresholds of the BVH kernel (no effect on results; rayz_hip_debug_set refuses values outside 1 .. 64 lanes)
    A.bvh_keep = (uint32_t)tuning(RAYZ_DEBUG_BVH_KEEP, kBvhKeepActive | (kBvhKeepStepping << 8));

    BvhLaunchPlan<R> plan{};
    plan.kernel = trace_kernel<R, 1>;
    plan.block = 256;
    plan.items_per_lane = 1;
    if (use_bvh) {
        plan.kernel = b.quantized ? trace_kernel_bvh<R, true> : trace_kernel_bvh<R, false>;
        plan.block = (int)kBvhWg;
        // the BVH kernel's LDS stack holds one entry per tree level below the root (nearer child first: the stack never
        // holds more than one entry per level); sized from THIS tree, so a shallow tree does not cap the occupancy
        // (+ one guard row under entry 0: a lane that has popped its sentinel reads ahead at index −1)
        plan.stack_bytes = ((size_t)s->bvh_dev.depth + 3) * kBvhWg * sizeof(uint32_t);
        // the tree's top: first in LDS.  The scene numbered b.bvh_top records breadth-first for this kernel's workgroup
        plan.top_records = b.bvh_top;
        rc = experiment_override<R>(plan, A, s, b, p); // (the product build: nothing)
        if (rc != RAYZ_OK) return rc;
    }
    experiment = plan.experiment;
    // The LDS request: top | stacks | oversized hittables' records (+ RAYZ_DEBUG_LDS_PAD unused bytes: an occupancy experiment —
    // fewer workgroups per CU, the same code), the top shortened should the request be refused (request_lds)
    const size_t big_bytes = use_bvh && b.n_big_leaves ? kBvhBigLdsBytes : 0;
    const size_t bvh_fixed = use_bvh ? plan.stack_bytes + big_bytes + plan.extra_lds_bytes + (size_t)tuning(RAYZ_DEBUG_LDS_PAD, 0) : 0;
    const size_t rec_bytes = b.quantized ? 32 : 64;
    size_t bvh_lds = 0;
    int blocks_per_cu = 0;
    rc = request_lds(plan.kernel, "trace", plan.block, rec_bytes, bvh_fixed, plan.top_records, bvh_lds, blocks_per_cu);
    if (rc != RAYZ_OK) return rc;
    const size_t bvh_top_bytes = (size_t)plan.top_records * rec_bytes;
    A.bvh_top_words = (uint32_t)(bvh_top_bytes / sizeof(uint32_t));
    A.bvh_big_words = (uint32_t)((bvh_top_bytes + plan.stack_bytes) / sizeof(uint32_t));
    A.sc.bvh_top = (uint32_t)bvh_top_bytes; // the walk compares byte offsets
    experiment_lds_placed<R>(A, (uint32_t)((bvh_top_bytes + plan.stack_bytes + big_bytes) / sizeof(uint32_t)));
    if (blocks_per_cu < 1) blocks_per_cu = 1;
    uint64_t grid = (uint64_t)ctx.num_cu * blocks_per_cu;
    const uint64_t per_block = (uint64_t)plan.items_per_lane * plan.block;
    const uint64_t want = (items64 + per_block - 1) / per_block;
    if (grid > want) grid = want;

    HIP_TRY(hipMemsetAsync(counters, 0, reset_bytes, stream));
    HIP_TRY(hipEventRecord(ev0, stream));
    hipLaunchKernelGGL(plan.kernel, dim3((uint32_t)grid), dim3(plan.block), bvh_lds, stream, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(ev1, stream));
    return RAYZ_OK;
}


// Launches one render of `p`'s shard on the scene's device: the trace kernel over every chunk, then resolve_kernel.  The caller
// has selected that device (DeviceScope).
template <class R>
int render_impl(RayzScene* s, const DeviceCtx& ctx, SceneBuffers<R>& b, const RayzCameraDesc* cam, const RayzRenderParams* p,
                R* d_out, hipStream_t stream) {
    typedef typename VecOf<R>::type r4;
    bool use_bvh = false;
    int rc = prepare_scene<R>(s, b, cam, p, stream, use_bvh);
    if (rc != RAYZ_OK) return rc;

    const uint32_t rows = rayz_hip_shard_rows(p);
    const uint64_t shard_pixels64 = (uint64_t)rows * p->width;
    std::vector<uint32_t> starts;
    chunk_schedule(p, starts);
    const uint32_t chunks_per_px = (uint32_t)starts.size() - 1;
    const uint64_t items64 = shard_pixels64 * chunks_per_px;
    rc = check_items(shard_pixels64, chunks_per_px);
    if (rc != RAYZ_OK) return rc;
    s->last = RayzRenderStats{};
    s->last.primary_rays = shard_pixels64 * p->samples_per_px;
    s->last_bvh = use_bvh;
    s->last_experiment = 0;
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
    if (starts != s->chunk_start_host) { // the schedule table, kept on the device until it changes
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(s->chunk_start.grow(starts.size()));
        HIP_TRY(hipMemcpy(s->chunk_start, starts.data(), starts.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        s->chunk_start_host = starts;
    }
    if (!s->ev0) {
        HIP_TRY(s->ev0.create());
        HIP_TRY(s->ev1.create());
    }
    rc = trace_window<R>(s, ctx, b, cam, p, use_bvh, starts, s->chunk_start, 0, chunks_per_px, s->counters,
                         32 * sizeof(unsigned long long), s->ev0, s->ev1, stream, s->last_experiment);
    if (rc != RAYZ_OK) return rc;
    hipLaunchKernelGGL(resolve_kernel<R>, dim3((uint32_t)((shard_pixels64 + 255) / 256)), dim3(256), 0, stream,
                       (const r4*)s->partial.get(), d_out, (uint32_t)shard_pixels64, chunks_per_px, p->samples_per_px);
    HIP_TRY(hipGetLastError());
    s->rendered = true;
    return RAYZ_OK;
}

int check_render_args(RayzScene* s, const RayzCameraDesc* cam, const RayzRenderParams* p, uint32_t precision) {
    if (!s) return fail(RAYZ_ERR_STATE, "scene handle is null");
    if (!cam) return fail(RAYZ_ERR_BAD_ARG, "camera is null");
    int rc = validate_params(p);
    if (rc != RAYZ_OK) return rc;
    if (p->precision != precision)
        return fail(RAYZ_ERR_BAD_ARG, "params.precision %u does not match this entry point", p->precision);
    return RAYZ_OK;
}

template <class R>
int render_device(RayzScene* s, const RayzCameraDesc* cam, const RayzRenderParams* p, R* d_out, void* stream, uint32_t precision) {
    int rc = check_render_args(s, cam, p, precision);
    if (rc != RAYZ_OK) return rc;
    DeviceCtx* ctx = nullptr;
    rc = scene_ctx(s, &ctx);
    if (rc != RAYZ_OK) return rc;
    DeviceScope scope(s->device);
    return render_impl<R>(s, *ctx, buffers_of<R>(*s), cam, p, d_out, stream ? (hipStream_t)stream : ctx->stream);
}

// (a handle is built in a unique_ptr and released to the caller at the end: an exception on the way, which guarded() reports,
// takes the half-built handle with it)
int scene_new(const RayzSceneDesc* scene, int device, std::unique_ptr<RayzScene>& out) {
    const int rc = validate_scene(scene);
    if (rc != RAYZ_OK) return rc;
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

int scene_sync(RayzScene* s, RayzRenderStats* stats) {
    if (!s) return fail(RAYZ_ERR_STATE, "scene handle is null");
    if (s->device < 0) { // never rendered: nothing to wait for
        if (stats) *stats = s->last;
        return RAYZ_OK;
    }
    DeviceScope scope(s->device);
    if (s->last_stream) HIP_TRY(hipStreamSynchronize(s->last_stream));
    if (s->rendered) {
        unsigned long long c[32] = {};
        HIP_TRY(hipMemcpy(c, s->counters, sizeof(c), hipMemcpyDeviceToHost));
#ifdef RAYZ_FLAT_PROFILE // measurement build only: wave time per phase of trace_kernel
        if (!s->last_bvh && c[9]) {
            const double tot = (double)(c[4] + c[5] + c[6] + c[7] + c[8]);
            std::fprintf(stderr, "flat phases (share of wave time; ticks per wave-iteration %.0f): refill %.1f%% | setup %.1f%% | scan %.1f%% | "
                                 "flush %.1f%% | shade %.1f%%\n", tot / (double)c[9], 100.0 * c[4] / tot, 100.0 * c[5] / tot,
                         100.0 * c[6] / tot, 100.0 * c[7] / tot, 100.0 * c[8] / tot);
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
        if (s->last_experiment) { // a retired kernel ran: its phase profile (measurement builds) and its abort flag
            const int rc = experiment_sync(s->last_experiment, c);
            if (rc != RAYZ_OK) return rc;
        }
        if (s->last_bvh && c[31])
            return fail(RAYZ_ERR_STATE, "trace_kernel_bvh refused to run: its dynamic LDS segment does not start at LDS address 0");
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
        s->last.segments = c[1];
        s->last.sphere_tests = s->last_bvh ? c[3] : c[1] * (unsigned long long)(s->spheres.size() + s->triangles.size());
        s->last.node_tests = s->last_bvh ? c[2] : 0;
        s->last.kernel_ms = ms;
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
    int rc = validate_params(p);
    if (rc != RAYZ_OK) return rc;
    int device;
    {
        std::unique_lock<std::mutex> lock(g_mu);
        device = g_default;
    }
    if (device < 0) {
        rc = rayz_hip_init(0);
        if (rc != RAYZ_OK) return rc;
        device = 0;
    }
    std::unique_ptr<RayzScene> s;
    rc = scene_new(scene, device, s);
    if (rc != RAYZ_OK) return rc;
    DeviceScope scope(device);
    const size_t n = (size_t)rayz_hip_shard_rows(p) * p->width * 3;
    DevBuf<R> d_out; // (declared after the scene: freed first, as ever)
    hipError_t e = d_out.alloc(n);
    if (e != hipSuccess) return fail(RAYZ_ERR_OOM, "hipMalloc(output): %s", hipGetErrorString(e));
    rc = render_device<R>(s.get(), cam, p, d_out.get(), nullptr, precision);
    if (rc == RAYZ_OK) rc = scene_sync(s.get(), stats);
    if (rc == RAYZ_OK && n) {
        e = hipMemcpy(out, d_out, n * sizeof(R), hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = fail(RAYZ_ERR_HIP, "hipMemcpy(output): %s", hipGetErrorString(e));
    }
    return rc;
}

// ---- progressive rendering (rayz_hip_progressive_*): the frame in passes of whole chunks ---------------------------------
// A pass traces a window of chunks [c0, c1) into the scene's workspace and folds the window's chunk sums into the handle's
// accumulator in chunk order (accumulate_kernel).  The chunk sums do not depend on the window (trace_window), and the fold
// performs resolve_kernel's additions in resolve_kernel's order, so once every chunk is covered the frame is the one-shot
// render's, bit for bit, whatever the passes were.
} // namespace

struct RayzProgressive {
    RayzScene* scene = nullptr;
    int device = -1;
    RayzCameraDesc cam{};
    RayzRenderParams params{};
    std::vector<uint32_t> starts;           // the chunk schedule: n_chunks + 1 entries
    DevBuf<uint32_t> d_starts;              // the handle's own device copy (the scene's table follows the scene's last render)
    DevBytes acc;                           // shard_pixels running sums (r4 of the precision)
    DevBuf<unsigned long long> counters;    // [0] queue head (cleared per pass), [1..3] summed over the passes
    uint64_t shard_pixels = 0;
    uint32_t chunks_done = 0;
    uint64_t primary_rays = 0;
    bool bvh = false, traced = false;
    std::vector<DevEvent> pending, spare;   // pairs bracketing the trace kernel of every pass not yet summed into kernel_ms
    double kernel_ms = 0;
    hipStream_t last_stream = nullptr;
    // noise tracking (rayz_hip_progressive_track_noise): absent from an untracked handle
    bool tracked = false;
    DevBuf<d4> q;                           // shard_pixels records {Q_r, Q_g, Q_b, 0}
    DevBuf<unsigned long long> nz_summary;  // [0] unconverged pixels, [1] max rel2 (bit pattern): cleared per evaluation
    DevBuf<double> nz_block_sum;            // Σ finite var per block of noise_eval_kernel
    DevEvent pass_done;                     // recorded behind every pass: what an evaluation on another stream waits for
    hipStream_t noise_stream = nullptr;     // the stream of the last evaluation (it reads acc and q: the next pass waits for it)
    ~RayzProgressive() { // the accumulator's last pass, and the last evaluation, have finished before the members go
        if (device < 0) return;
        DeviceScope scope(device);
        if (last_stream) (void)hipStreamSynchronize(last_stream);
        if (noise_stream && noise_stream != last_stream) (void)hipStreamSynchronize(noise_stream);
    }
};

namespace {

int progressive_free(RayzProgressive* pr) {
    delete pr;
    return RAYZ_OK;
}

int progressive_create(RayzScene* s, const RayzCameraDesc* cam, const RayzRenderParams* p, RayzProgressive** out) {
    if (!out) return fail(RAYZ_ERR_BAD_ARG, "out handle pointer is null");
    *out = nullptr;
    if (!s) return fail(RAYZ_ERR_STATE, "scene handle is null");
    if (!p) return fail(RAYZ_ERR_BAD_ARG, "params is null");
    int rc = check_render_args(s, cam, p, p->precision); // (either precision: the step entry must then match it)
    if (rc != RAYZ_OK) return rc;
    const uint64_t shard_pixels = (uint64_t)rayz_hip_shard_rows(p) * p->width;
    rc = check_items(shard_pixels, 1);
    if (rc != RAYZ_OK) return rc;
    DeviceCtx* ctx = nullptr;
    rc = scene_ctx(s, &ctx);
    if (rc != RAYZ_OK) return rc;
    std::vector<uint32_t> starts;
    chunk_schedule(p, starts);
    DeviceScope scope(s->device);
    auto pr = std::make_unique<RayzProgressive>();
    pr->scene = s;
    pr->device = s->device;
    pr->cam = *cam;
    pr->params = *p;
    pr->shard_pixels = shard_pixels;
    pr->starts.swap(starts);
    const size_t r4_bytes = p->precision == RAYZ_PRECISION_F64 ? sizeof(d4) : sizeof(f4);
    hipError_t e = pr->d_starts.upload(pr->starts);
    if (e == hipSuccess) e = pr->acc.alloc(shard_pixels * r4_bytes);
    if (e == hipSuccess) e = pr->counters.alloc(32);
    if (e == hipSuccess) e = hipMemset(pr->counters, 0, 32 * sizeof(unsigned long long));
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? RAYZ_ERR_OOM : RAYZ_ERR_HIP, "progressive handle: %s", hipGetErrorString(e));
    *out = pr.release();
    return RAYZ_OK;
}

template <class R>
int progressive_step(RayzProgressive* pr, uint32_t min_samples, R* d_preview, void* stream_arg, uint32_t precision) {
    typedef typename VecOf<R>::type r4;
    if (!pr) return fail(RAYZ_ERR_STATE, "progressive handle is null");
    if (pr->params.precision != precision)
        return fail(RAYZ_ERR_BAD_ARG, "params.precision %u does not match this entry point", pr->params.precision);
    const uint32_t n = (uint32_t)pr->starts.size() - 1, c0 = pr->chunks_done;
    if (c0 >= n) return fail(RAYZ_ERR_STATE, "the progressive render is finished (%u of %u chunks done)", c0, n);
    // the fewest whole chunks from the cursor that add at least min_samples samples (at least one, at most the rest)
    const uint64_t want = (uint64_t)pr->starts[c0] + min_samples;
    uint32_t c1 = (uint32_t)(std::lower_bound(pr->starts.begin() + c0 + 1, pr->starts.end(), want) - pr->starts.begin());
    if (c1 > n) c1 = n;
    RayzScene* s = pr->scene;
    DeviceCtx* ctx = nullptr;
    int rc = scene_ctx(s, &ctx);
    if (rc != RAYZ_OK) return rc;
    DeviceScope scope(s->device);
    const hipStream_t stream = stream_arg ? (hipStream_t)stream_arg : ctx->stream;
    SceneBuffers<R>& b = buffers_of<R>(*s);
    bool use_bvh = false;
    rc = prepare_scene<R>(s, b, &pr->cam, &pr->params, stream, use_bvh);
    if (rc != RAYZ_OK) return rc;
    rc = check_items(pr->shard_pixels, c1 - c0);
    if (rc != RAYZ_OK) return rc;
    if (pr->last_stream && pr->last_stream != stream) HIP_TRY(hipStreamSynchronize(pr->last_stream)); // the accumulator's last pass
    if (pr->noise_stream && pr->noise_stream != stream) HIP_TRY(hipStreamSynchronize(pr->noise_stream)); // .. and its last reader
    pr->bvh = use_bvh;
    const uint64_t samples = pr->starts[c1] - pr->starts[c0];
    if (pr->shard_pixels && pr->params.max_bounces == 0) { // bounceRay(ray, 0) is black, src/renderer.zig:104-105
        if (d_preview) HIP_TRY(hipMemsetAsync(d_preview, 0, pr->shard_pixels * 3 * sizeof(R), stream));
        pr->last_stream = stream;
    } else if (pr->shard_pixels) {
        if (!s->counters) HIP_TRY(s->counters.alloc(32)); // (the scene's: left alone)
        while (pr->spare.size() < 2) {
            DevEvent e;
            HIP_TRY(e.create());
            pr->spare.push_back(std::move(e));
        }
        DevEvent ev1 = std::move(pr->spare.back());
        pr->spare.pop_back();
        DevEvent ev0 = std::move(pr->spare.back());
        pr->spare.pop_back();
        s->last_stream = stream;
        pr->last_stream = stream;
        int experiment = 0; // (the passes' counters are not reported)
        rc = trace_window<R>(s, *ctx, b, &pr->cam, &pr->params, use_bvh, pr->starts, pr->d_starts, c0, c1, pr->counters,
                             sizeof(unsigned long long), ev0, ev1, stream, experiment);
        if (rc != RAYZ_OK) {
            pr->spare.push_back(std::move(ev0));
            pr->spare.push_back(std::move(ev1));
            return rc;
        }
        pr->pending.push_back(std::move(ev0));
        pr->pending.push_back(std::move(ev1));
        if (pr->tracked)
            hipLaunchKernelGGL(accumulate_moments_kernel<R>, dim3((uint32_t)((pr->shard_pixels + 255) / 256)), dim3(256), 0, stream,
                               (const r4*)s->partial.get(), (r4*)pr->acc.get(), pr->q.get(), d_preview, pr->d_starts.get() + c0,
                               (uint32_t)pr->shard_pixels, c1 - c0, pr->starts[c1], c0 == 0 ? 1u : 0u);
        else
            hipLaunchKernelGGL(accumulate_kernel<R>, dim3((uint32_t)((pr->shard_pixels + 255) / 256)), dim3(256), 0, stream,
                               (const r4*)s->partial.get(), (r4*)pr->acc.get(), d_preview, (uint32_t)pr->shard_pixels, c1 - c0,
                               pr->starts[c1], c0 == 0 ? 1u : 0u);
        HIP_TRY(hipGetLastError());
        pr->traced = true;
    }
    if (pr->tracked && pr->shard_pixels) HIP_TRY(hipEventRecord(pr->pass_done, stream));
    pr->primary_rays += pr->shard_pixels * samples;
    pr->chunks_done = c1;
    return RAYZ_OK;
}

int progressive_info(const RayzProgressive* cpr, uint32_t* samples_done, uint32_t* chunks_done, uint32_t* n_chunks,
                     RayzRenderStats* total) {
    if (!cpr) return fail(RAYZ_ERR_STATE, "progressive handle is null");
    RayzProgressive* pr = const_cast<RayzProgressive*>(cpr); // (summing the passes' kernel times recycles their events)
    if (samples_done) *samples_done = pr->starts[pr->chunks_done];
    if (chunks_done) *chunks_done = pr->chunks_done;
    if (n_chunks) *n_chunks = (uint32_t)pr->starts.size() - 1;
    if (!total) return RAYZ_OK;
    RayzRenderStats st{};
    st.primary_rays = pr->primary_rays;
    if (pr->noise_stream) { // .. and for the last evaluation: what a caller of rayz_hip_progressive_noise without a summary waits with
        DeviceScope scope(pr->device);
        HIP_TRY(hipStreamSynchronize(pr->noise_stream));
    }
    if (pr->traced) {
        DeviceScope scope(pr->device);
        if (pr->last_stream) HIP_TRY(hipStreamSynchronize(pr->last_stream));
        unsigned long long c[32] = {};
        HIP_TRY(hipMemcpy(c, pr->counters, sizeof(c), hipMemcpyDeviceToHost));
        if (pr->bvh && c[31])
            return fail(RAYZ_ERR_STATE, "trace_kernel_bvh refused to run: its dynamic LDS segment does not start at LDS address 0");
        for (size_t i = 0; i + 1 < pr->pending.size(); i += 2) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, pr->pending[i], pr->pending[i + 1]));
            pr->kernel_ms += ms;
        }
        for (DevEvent& e : pr->pending) pr->spare.push_back(std::move(e));
        pr->pending.clear();
        const RayzScene* s = pr->scene;
        st.segments = c[1];
        st.sphere_tests = pr->bvh ? c[3] : c[1] * (unsigned long long)(s->spheres.size() + s->triangles.size());
        st.node_tests = pr->bvh ? c[2] : 0;
        st.kernel_ms = pr->kernel_ms;
    }
    *total = st;
    return RAYZ_OK;
}

// ---- the noise estimate of a tracked handle (kernels: noise.hpp) ------------------------------------------------
int noise_params(const RayzNoiseParams* in, double& tau2, double& floor2) {
    const RayzNoiseParams p = in ? *in : RayzNoiseParams{RAYZ_NOISE_DEFAULT_REL_ERROR, RAYZ_NOISE_DEFAULT_MEAN_FLOOR};
    tau2 = p.rel_error * p.rel_error, floor2 = p.mean_floor * p.mean_floor; // (f64, rounded once each: what the kernel compares with)
    if (!(p.rel_error > 0) || !(tau2 > 0)) return fail(RAYZ_ERR_BAD_ARG, "noise rel_error %g: must be positive (and its square)", p.rel_error);
    if (!(p.mean_floor > 0) || !(floor2 > 0)) return fail(RAYZ_ERR_BAD_ARG, "noise mean_floor %g: must be positive (and its square)", p.mean_floor);
    return RAYZ_OK;
}

int progressive_track_noise(RayzProgressive* pr) {
    if (!pr) return fail(RAYZ_ERR_STATE, "progressive handle is null");
    if (pr->tracked) return RAYZ_OK;
    if (pr->chunks_done) return fail(RAYZ_ERR_STATE, "noise tracking starts before the first step (%u chunks done)", pr->chunks_done);
    DeviceScope scope(pr->device);
    const size_t r4_bytes = pr->params.precision == RAYZ_PRECISION_F64 ? sizeof(d4) : sizeof(f4);
    const uint32_t blocks = noise_blocks(pr->shard_pixels);
    hipError_t e = pr->q.alloc(pr->shard_pixels);
    if (e == hipSuccess) e = pr->nz_summary.alloc(2);
    if (e == hipSuccess) e = pr->nz_block_sum.alloc(blocks);
    if (e == hipSuccess) e = pr->pass_done.create(hipEventDisableTiming);
    // +0 everywhere: what an evaluation before the first pass — or of a render whose passes trace nothing (max_bounces = 0) — reads
    if (e == hipSuccess && pr->shard_pixels) e = hipMemset(pr->q, 0, pr->shard_pixels * sizeof(d4));
    if (e == hipSuccess && pr->shard_pixels) e = hipMemset(pr->acc, 0, pr->shard_pixels * r4_bytes);
    if (e != hipSuccess) {
        pr->q.reset();
        return fail(e == hipErrorOutOfMemory ? RAYZ_ERR_OOM : RAYZ_ERR_HIP, "noise state: %s", hipGetErrorString(e));
    }
    pr->tracked = true;
    return RAYZ_OK;
}

// Launches noise_eval_kernel on `stream` and, with `summary`, waits for it and fills the summary.  `acc`, `q`: `pixels` records.
template <class R>
int noise_eval(const void* acc, const d4* q, float* d_var, float* d_rel2, double* d_var64, double* d_rel264, unsigned long long* d_summary,
               double* d_block_sum, uint64_t pixels, uint32_t chunks_done, uint32_t samples_done, double floor2, double tau2,
               RayzNoiseSummary* summary, hipStream_t stream) {
    typedef typename VecOf<R>::type r4;
    const uint32_t blocks = noise_blocks(pixels);
    if (pixels) {
        HIP_TRY(hipMemsetAsync(d_summary, 0, 2 * sizeof(unsigned long long), stream));
        hipLaunchKernelGGL(noise_eval_kernel<R>, dim3(blocks), dim3(256), 0, stream, (const r4*)acc, q, d_var, d_rel2, d_var64, d_rel264,
                           d_summary, d_block_sum, (uint32_t)pixels, chunks_done, samples_done, floor2, tau2);
        HIP_TRY(hipGetLastError());
    }
    if (!summary) return RAYZ_OK;
    RayzNoiseSummary out{};
    out.pixels = pixels, out.samples_done = samples_done, out.chunks_done = chunks_done;
    if (pixels) {
        unsigned long long two[2] = {0, 0};
        std::vector<double> part(blocks);
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(hipMemcpy(two, d_summary, sizeof(two), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(part.data(), d_block_sum, blocks * sizeof(double), hipMemcpyDeviceToHost));
        double sum = 0.0;
        for (const double x : part) sum = sum + x; // block order
        out.unconverged = two[0];
        std::memcpy(&out.max_rel2, &two[1], sizeof(double));
        out.mean_var = sum / (double)pixels;
    }
    *summary = out;
    return RAYZ_OK;
}

int progressive_noise(RayzProgressive* pr, const RayzNoiseParams* params, float* d_var, float* d_rel2, RayzNoiseSummary* summary,
                      void* stream_arg) {
    double tau2 = 0, floor2 = 0;
    int rc = noise_params(params, tau2, floor2);
    if (rc != RAYZ_OK) return rc;
    if (!pr) return fail(RAYZ_ERR_STATE, "progressive handle is null");
    if (!pr->tracked) return fail(RAYZ_ERR_STATE, "the handle does not track noise (rayz_hip_progressive_track_noise before the first step)");
    DeviceCtx* ctx = nullptr;
    rc = scene_ctx(pr->scene, &ctx);
    if (rc != RAYZ_OK) return rc;
    DeviceScope scope(pr->device);
    const hipStream_t stream = stream_arg ? (hipStream_t)stream_arg : ctx->stream;
    if (pr->noise_stream && pr->noise_stream != stream) HIP_TRY(hipStreamSynchronize(pr->noise_stream)); // one evaluation owns the summary
    if (pr->last_stream && pr->last_stream != stream && pr->shard_pixels) HIP_TRY(hipStreamWaitEvent(stream, pr->pass_done, 0));
    pr->noise_stream = stream;
    const uint32_t K = pr->chunks_done, N = pr->starts[K];
    if (pr->params.precision == RAYZ_PRECISION_F64)
        return noise_eval<double>(pr->acc.get(), pr->q, d_var, d_rel2, nullptr, nullptr, pr->nz_summary, pr->nz_block_sum, pr->shard_pixels, K,
                                  N, floor2, tau2, summary, stream);
    return noise_eval<float>(pr->acc.get(), pr->q, d_var, d_rel2, nullptr, nullptr, pr->nz_summary, pr->nz_block_sum, pr->shard_pixels, K, N,
                             floor2, tau2, summary, stream);
}

int progressive_noise_state(RayzProgressive* pr, double* d_q, void* stream_arg) {
    if (!pr) return fail(RAYZ_ERR_STATE, "progressive handle is null");
    if (!pr->tracked) return fail(RAYZ_ERR_STATE, "the handle does not track noise (rayz_hip_progressive_track_noise before the first step)");
    if (!pr->shard_pixels) return RAYZ_OK;
    if (!d_q) return fail(RAYZ_ERR_BAD_ARG, "null buffer");
    DeviceCtx* ctx = nullptr;
    const int rc = scene_ctx(pr->scene, &ctx);
    if (rc != RAYZ_OK) return rc;
    DeviceScope scope(pr->device);
    const hipStream_t stream = stream_arg ? (hipStream_t)stream_arg : ctx->stream;
    if (pr->noise_stream && pr->noise_stream != stream) HIP_TRY(hipStreamSynchronize(pr->noise_stream));
    if (pr->last_stream && pr->last_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, pr->pass_done, 0));
    pr->noise_stream = stream; // (a reader of q, as an evaluation is)
    HIP_TRY(hipMemcpyAsync(d_q, pr->q, pr->shard_pixels * sizeof(d4), hipMemcpyDeviceToDevice, stream));
    HIP_TRY(hipStreamSynchronize(stream)); // (an accessor for tests and tools: it blocks)
    return RAYZ_OK;
}

template <class R>
int progressive_run_until(RayzProgressive* pr, const RayzNoiseParams* params, double max_fraction, uint32_t min_samples, R* d_preview,
                          RayzNoiseSummary* last, void* stream_arg, uint32_t precision) {
    double tau2 = 0, floor2 = 0;
    int rc = noise_params(params, tau2, floor2);
    if (rc != RAYZ_OK) return rc;
    if (!(max_fraction >= 0.0 && max_fraction <= 1.0))
        return fail(RAYZ_ERR_BAD_ARG, "max_unconverged_fraction %g: must lie in [0, 1]", max_fraction);
    if (!pr) return fail(RAYZ_ERR_STATE, "progressive handle is null");
    if (!pr->tracked) return fail(RAYZ_ERR_STATE, "the handle does not track noise (rayz_hip_progressive_track_noise before the first step)");
    const uint32_t n = (uint32_t)pr->starts.size() - 1;
    RayzNoiseSummary sm{};
    for (;;) {
        rc = progressive_step<R>(pr, min_samples, d_preview, stream_arg, precision);
        if (rc != RAYZ_OK) return rc;
        rc = progressive_noise(pr, params, nullptr, nullptr, &sm, stream_arg);
        if (rc != RAYZ_OK) return rc;
        if ((double)sm.unconverged <= max_fraction * (double)sm.pixels || pr->chunks_done >= n) break;
    }
    if (last) *last = sm;
    return RAYZ_OK;
}

int noise_kat(uint32_t precision, const double* sums, const uint32_t* sizes, uint32_t n_pixels, uint32_t n_chunks,
              const RayzNoiseParams* params, double* q_out, double* var_out, double* rel2_out, RayzNoiseSummary* summary) {
    double tau2 = 0, floor2 = 0;
    int rc = noise_params(params, tau2, floor2);
    if (rc != RAYZ_OK) return rc;
    if (precision > RAYZ_PRECISION_F64) return fail(RAYZ_ERR_BAD_ARG, "bad precision %u", precision);
    if (!n_chunks) return fail(RAYZ_ERR_BAD_ARG, "n_chunks is 0");
    if (!sizes || (n_pixels && !sums)) return fail(RAYZ_ERR_BAD_ARG, "null buffer");
    if ((uint64_t)n_pixels * n_chunks > (1ull << 28)) return fail(RAYZ_ERR_BAD_ARG, "n_pixels x n_chunks = %llu: more than 2^28 chunk sums",
                                                                   (unsigned long long)n_pixels * n_chunks);
    std::vector<uint32_t> starts(n_chunks + 1, 0);
    for (uint32_t k = 0; k < n_chunks; ++k) {
        if (!sizes[k] || (uint64_t)starts[k] + sizes[k] > UINT32_MAX)
            return fail(RAYZ_ERR_BAD_ARG, "chunk_sizes[%u] = %u: a chunk holds at least one sample, and all of them at most 2^32 - 1", k, sizes[k]);
        starts[k + 1] = starts[k] + sizes[k];
    }
    int device;
    hipStream_t stream;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        device = g_default;
        if (device < 0) return fail(RAYZ_ERR_NO_DEVICE, "rayz_hip_init has not succeeded");
        stream = g_ctx[device].stream;
    }
    if (!n_pixels) {
        if (summary) *summary = RayzNoiseSummary{0, 0, 0.0, 0.0, starts[n_chunks], n_chunks};
        return RAYZ_OK;
    }
    const bool f64 = precision == RAYZ_PRECISION_F64;
    const size_t items = (size_t)n_pixels * n_chunks, r4_bytes = f64 ? sizeof(d4) : sizeof(f4);
    std::vector<char> host(items * r4_bytes); // the chunk-sum records a trace pass would have left
    for (size_t i = 0; i < items; ++i) {
        if (f64) reinterpret_cast<d4*>(host.data())[i] = d4{sums[3 * i], sums[3 * i + 1], sums[3 * i + 2], 0.0};
        else reinterpret_cast<f4*>(host.data())[i] = f4{(float)sums[3 * i], (float)sums[3 * i + 1], (float)sums[3 * i + 2], 0.0f};
    }
    DeviceScope scope(device);
    DevBytes d_partial, d_acc;
    DevBuf<d4> d_q;
    DevBuf<uint32_t> d_starts;
    DevBuf<double> d_var, d_rel2, d_block_sum;
    DevBuf<unsigned long long> d_summary;
    const uint32_t blocks = noise_blocks(n_pixels);
    hipError_t e = d_partial.alloc(host.size());
    if (e == hipSuccess) e = d_acc.alloc(n_pixels * r4_bytes);
    if (e == hipSuccess) e = d_q.alloc(n_pixels);
    if (e == hipSuccess) e = d_starts.upload(starts);
    if (e == hipSuccess) e = d_var.alloc(n_pixels);
    if (e == hipSuccess) e = d_rel2.alloc(n_pixels);
    if (e == hipSuccess) e = d_block_sum.alloc(blocks);
    if (e == hipSuccess) e = d_summary.alloc(2);
    if (e == hipSuccess) e = hipMemcpyAsync(d_partial, host.data(), host.size(), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? RAYZ_ERR_OOM : RAYZ_ERR_HIP, "rayz_hip_noise_kat: %s", hipGetErrorString(e));
    // the fold as two passes: chunk 0 from +0, then the rest onto acc and q
    for (uint32_t pass = 0; pass < (n_chunks > 1 ? 2u : 1u); ++pass) {
        const uint32_t c0 = pass, c1 = pass ? n_chunks : 1;
        const char* src = d_partial.get() + (size_t)c0 * n_pixels * r4_bytes;
        if (f64)
            hipLaunchKernelGGL(accumulate_moments_kernel<double>, dim3(blocks), dim3(256), 0, stream, (const d4*)src, (d4*)d_acc.get(), d_q.get(),
                               (double*)nullptr, d_starts.get() + c0, n_pixels, c1 - c0, starts[c1], pass ? 0u : 1u);
        else
            hipLaunchKernelGGL(accumulate_moments_kernel<float>, dim3(blocks), dim3(256), 0, stream, (const f4*)src, (f4*)d_acc.get(), d_q.get(),
                               (float*)nullptr, d_starts.get() + c0, n_pixels, c1 - c0, starts[c1], pass ? 0u : 1u);
        HIP_TRY(hipGetLastError());
    }
    RayzNoiseSummary sm{};
    rc = f64 ? noise_eval<double>(d_acc.get(), d_q, nullptr, nullptr, d_var, d_rel2, d_summary, d_block_sum, n_pixels, n_chunks, starts[n_chunks],
                                  floor2, tau2, &sm, stream)
             : noise_eval<float>(d_acc.get(), d_q, nullptr, nullptr, d_var, d_rel2, d_summary, d_block_sum, n_pixels, n_chunks, starts[n_chunks],
                                 floor2, tau2, &sm, stream);
    if (rc != RAYZ_OK) return rc; // (noise_eval has waited for the stream)
    if (q_out) {
        std::vector<d4> q(n_pixels);
        HIP_TRY(hipMemcpy(q.data(), d_q, n_pixels * sizeof(d4), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n_pixels; ++i) q_out[3 * i] = q[i].x, q_out[3 * i + 1] = q[i].y, q_out[3 * i + 2] = q[i].z;
    }
    if (var_out) HIP_TRY(hipMemcpy(var_out, d_var, n_pixels * sizeof(double), hipMemcpyDeviceToHost));
    if (rel2_out) HIP_TRY(hipMemcpy(rel2_out, d_rel2, n_pixels * sizeof(double), hipMemcpyDeviceToHost));
    if (summary) *summary = sm;
    return RAYZ_OK;
}

// ---- RCCL, opened at run time ------------------------------------------------------------------------------
// The single-device entry points must not depend on RCCL being loadable, and a host that already carries an RCCL
// (torch ships one with the same soname) must not get a second copy: dlopen by soname reuses what is mapped.
struct Rccl {
    void* handle = nullptr;
    bool tried = false;
    decltype(&ncclGetVersion) GetVersion = nullptr;
    decltype(&ncclCommInitAll) CommInitAll = nullptr;
    decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGroupStart) GroupStart = nullptr;
    decltype(&ncclGroupEnd) GroupEnd = nullptr;
    decltype(&ncclGather) Gather = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
Rccl g_rccl;

int rccl_load() { // g_mu held
    Rccl& r = g_rccl;
    if (r.handle) return RAYZ_OK;
    if (r.tried) return fail(RAYZ_ERR_STATE, "RCCL is not available (librccl.so.1 could not be loaded)");
    r.tried = true;
    const char* names[] = {"librccl.so.1", "/opt/rocm/lib/librccl.so.1", "librccl.so"};
    void* h = nullptr;
    for (const char* n : names)
        if ((h = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    if (!h) return fail(RAYZ_ERR_STATE, "RCCL is not available: %s", dlerror());
    bool ok = true;
    auto sym = [&](const char* name) {
        void* p = dlsym(h, name);
        if (!p) ok = false;
        return p;
    };
    r.GetVersion = (decltype(r.GetVersion))sym("ncclGetVersion");
    r.CommInitAll = (decltype(r.CommInitAll))sym("ncclCommInitAll");
    r.CommDestroy = (decltype(r.CommDestroy))sym("ncclCommDestroy");
    r.GroupStart = (decltype(r.GroupStart))sym("ncclGroupStart");
    r.GroupEnd = (decltype(r.GroupEnd))sym("ncclGroupEnd");
    r.Gather = (decltype(r.Gather))sym("ncclGather");
    r.GetErrorString = (decltype(r.GetErrorString))sym("ncclGetErrorString");
    if (!ok) {
        dlclose(h);
        return fail(RAYZ_ERR_STATE, "RCCL is not available: librccl lacks a required symbol");
    }
    r.handle = h;
    return RAYZ_OK;
}

#define NCCL_TRY(expr)                                                                                      \
    do {                                                                                                    \
        ncclResult_t r_ = (expr);                                                                           \
        if (r_ != ncclSuccess)                                                                              \
            return fail(RAYZ_ERR_HIP, "%s: %s (%s:%d)", #expr, g_rccl.GetErrorString(r_), __FILE__, __LINE__); \
    } while (0)

// Interleaved row tiles back into the frame: gathered[rank][local row][w*3] -> frame[row][w*3] (on the root device).
template <class T>
__global__ __launch_bounds__(256) void unshard_kernel(const T* __restrict__ gathered, T* __restrict__ frame, uint32_t height,
                                                      uint32_t row_elems, uint32_t tile_rows, uint32_t n_ranks,
                                                      uint32_t max_rows) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)height * row_elems) return;
    const uint32_t y = (uint32_t)(i / row_elems), x = (uint32_t)(i - (size_t)y * row_elems);
    const uint32_t tile = y / tile_rows, rank = tile % n_ranks, local = (tile / n_ranks) * tile_rows + (y - tile * tile_rows);
    frame[i] = gathered[((size_t)rank * max_rows + local) * row_elems + x];
}

} // namespace

// One scene per device + the buffers of the gather; everything is driven by the calling host thread.
struct RayzMulti {
    std::vector<int> devices;
    // one entry per device, from construction on
    std::vector<std::unique_ptr<RayzScene>> scenes;
    std::vector<ncclComm_t> comms; // RAYZ_GATHER_RCCL (else null)
    std::vector<DevBytes> tile;    // this device's rows, grow-only
    std::vector<DevBytes> tile8;   // the same rows tone-mapped to u8 (render_u8 only)
    std::vector<DevEvent> done;    // tile ready (peer-copy transport)
    DevBytes gathered; // root: [n][max_rows][row bytes]
    DevBytes frame;    // root: the assembled frame
    uint32_t transport = RAYZ_GATHER_RCCL;
    int rccl_version = 0;
    std::vector<RayzRenderStats> last_dev; // per device: counters of the last frame (rayz_hip_multi_device_stats)
    DevEvent g0, g1; // on the root's stream: its own tile done / frame assembled
    double last_gather_ms = 0, last_frame_ms = 0;
    RayzMulti(const int* d, int n) : devices(d, d + n), scenes(n), comms(n, nullptr), tile(n), tile8(n), done(n) {}
    // Device by device: the scene (it waits for the device's last render), the communicator, the buffers; the root's own follow.
    ~RayzMulti() {
        for (size_t i = 0; i < devices.size(); ++i) {
            scenes[i].reset();
            if (comms[i]) {
                DeviceScope scope(devices[i]);
                (void)g_rccl.CommDestroy(comms[i]);
            }
            tile[i].reset(), tile8[i].reset(), done[i].reset();
        }
    }
};

namespace {

int multi_free(RayzMulti* m) {
    delete m;
    return RAYZ_OK;
}

// `dup_ok`: RAYZ_GATHER_ALLOW_DUPLICATE_DEVICES was passed with the peer-copy transport (tests on a one-GPU box: the N-way
// sharding, the gather into N slots and the un-interleave then run for real, every "device" being the same one)
int check_device_list(const int* devices, int n, bool dup_ok) {
    if (!devices) return fail(RAYZ_ERR_BAD_ARG, "device list is null");
    if (n < 1 || n > RAYZ_MAX_DEVICES) return fail(RAYZ_ERR_BAD_ARG, "n_devices %d out of range [1,%d]", n, RAYZ_MAX_DEVICES);
    for (int i = 0; i < n; ++i) {
        if (devices[i] < 0 || devices[i] >= RAYZ_MAX_DEVICES) return fail(RAYZ_ERR_BAD_ARG, "device %d out of range", devices[i]);
        for (int j = 0; j < i && !dup_ok; ++j)
            if (devices[j] == devices[i]) return fail(RAYZ_ERR_BAD_ARG, "device %d is listed twice", devices[i]);
    }
    return RAYZ_OK;
}

int multi_create(const int* devices, int n_devices, const RayzSceneDesc* scene, uint32_t transport, RayzMulti** out) {
    if (!out) return fail(RAYZ_ERR_BAD_ARG, "out handle pointer is null");
    *out = nullptr;
    const bool dup_ok = (transport & RAYZ_GATHER_ALLOW_DUPLICATE_DEVICES) != 0;
    transport &= ~(uint32_t)RAYZ_GATHER_ALLOW_DUPLICATE_DEVICES;
    if (transport > RAYZ_GATHER_PEER_COPY) return fail(RAYZ_ERR_BAD_ARG, "bad gather transport %u", transport);
    if (dup_ok && transport != RAYZ_GATHER_PEER_COPY)
        return fail(RAYZ_ERR_BAD_ARG, "RAYZ_GATHER_ALLOW_DUPLICATE_DEVICES needs the peer-copy transport (RCCL refuses a device twice)");
    int rc = check_device_list(devices, n_devices, dup_ok);
    if (rc != RAYZ_OK) return rc;
    rc = validate_scene(scene);
    if (rc != RAYZ_OK) return rc;
    {
        std::lock_guard<std::mutex> lock(g_mu);
        for (int i = 0; i < n_devices; ++i) {
            rc = ensure_ctx(devices[i]);
            if (rc != RAYZ_OK) return rc;
        }
        if (transport == RAYZ_GATHER_RCCL) {
            rc = rccl_load();
            if (rc != RAYZ_OK) return rc;
        }
    }
    auto m = std::make_unique<RayzMulti>(devices, n_devices);
    m->transport = transport;
    for (int i = 0; i < n_devices; ++i) {
        rc = scene_new(scene, devices[i], m->scenes[i]);
        if (rc != RAYZ_OK) return rc;
    }
    if (transport == RAYZ_GATHER_RCCL) {
        ncclResult_t r = g_rccl.CommInitAll(m->comms.data(), n_devices, m->devices.data());
        if (r != ncclSuccess) {
            m->comms.assign(n_devices, nullptr); // (whatever the failed call left there is no communicator to destroy)
            return fail(RAYZ_ERR_HIP, "ncclCommInitAll(%d devices): %s", n_devices, g_rccl.GetErrorString(r));
        }
        (void)g_rccl.GetVersion(&m->rccl_version);
    } else {
        for (int i = 0; i < n_devices; ++i) {
            DeviceScope scope(devices[i]);
            hipError_t e = m->done[i].create(hipEventDisableTiming);
            if (e != hipSuccess) return fail(RAYZ_ERR_HIP, "hipEventCreate: %s", hipGetErrorString(e));
            if (i > 0) { // the root pulls nothing; sources push into the root's buffer
                int can = 0;
                (void)hipDeviceCanAccessPeer(&can, devices[i], devices[0]);
                if (can) {
                    e = hipDeviceEnablePeerAccess(devices[0], 0);
                    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled)
                        return fail(RAYZ_ERR_HIP, "hipDeviceEnablePeerAccess(%d -> %d): %s", devices[i], devices[0], hipGetErrorString(e));
                    (void)hipGetLastError();
                }
            }
        }
    }
    *out = m.release();
    return RAYZ_OK;
}

// T = element type of the frame that crosses the ABI (float, double; uint8_t for the tone-mapped form, rendered in f32).
template <class T>
int multi_render(RayzMulti* m, const RayzCameraDesc* cam, const RayzRenderParams* p, T* out, RayzRenderStats* stats) {
    typedef typename std::conditional<sizeof(T) == 8, double, float>::type R;
    constexpr bool to_u8 = sizeof(T) == 1;
    if (!m) return fail(RAYZ_ERR_STATE, "multi handle is null");
    if (!cam) return fail(RAYZ_ERR_BAD_ARG, "camera is null");
    if (!out) return fail(RAYZ_ERR_BAD_ARG, "output pointer is null");
    int rc = validate_params(p);
    if (rc != RAYZ_OK) return rc;
    if (p->precision != (sizeof(R) == 8 ? RAYZ_PRECISION_F64 : RAYZ_PRECISION_F32))
        return fail(RAYZ_ERR_BAD_ARG, "params.precision %u does not match this entry point", p->precision);
    if (p->shard_index != 0 || p->shard_count > 1)
        return fail(RAYZ_ERR_BAD_ARG, "the multi-device entry shards the frame itself: shard_index / shard_count must be 0");
    const uint32_t n = (uint32_t)m->devices.size();
    RayzRenderParams q = *p;
    q.tile_rows = p->tile_rows ? p->tile_rows : RAYZ_DEFAULT_TILE_ROWS; // ONE default for every entry point (include/rayz_hip.h)
    q.shard_count = n;
    uint32_t max_rows = 0;
    for (uint32_t i = 0; i < n; ++i) {
        q.shard_index = i;
        const uint32_t r = rayz_hip_shard_rows(&q);
        max_rows = r > max_rows ? r : max_rows;
    }
    const size_t row_elems = (size_t)p->width * 3;
    const size_t tile_bytes = (size_t)max_rows * row_elems * sizeof(R), tile8_bytes = (size_t)max_rows * row_elems;
    const size_t send_bytes = to_u8 ? tile8_bytes : tile_bytes;
    const size_t frame_bytes = (size_t)p->height * row_elems * sizeof(T);
    if ((size_t)p->height * row_elems >= (1ull << 32)) return fail(RAYZ_ERR_BAD_ARG, "frame too large");

    // 1. every device traces its rows (asynchronous: the launches of all devices overlap)
    std::vector<DeviceCtx*> ctx(n, nullptr);
    for (uint32_t i = 0; i < n; ++i) {
        rc = scene_ctx(m->scenes[i].get(), &ctx[i]);
        if (rc != RAYZ_OK) return rc;
        DeviceScope scope(m->devices[i]);
        HIP_TRY(hipStreamSynchronize(ctx[i]->stream)); // the previous frame's gather has left the tiles
        HIP_TRY(m->tile[i].grow(tile_bytes ? tile_bytes : 16));
        if (to_u8) HIP_TRY(m->tile8[i].grow(tile8_bytes ? tile8_bytes : 16));
    }
    {
        DeviceScope scope(m->devices[0]);
        HIP_TRY(m->gathered.grow((size_t)n * send_bytes ? (size_t)n * send_bytes : 16));
        HIP_TRY(m->frame.grow(frame_bytes));
    }
    for (uint32_t i = 0; i < n; ++i) {
        DeviceScope scope(m->devices[i]);
        q.shard_index = i;
        rc = render_impl<R>(m->scenes[i].get(), *ctx[i], buffers_of<R>(*m->scenes[i]), cam, &q, (R*)m->tile[i].get(), ctx[i]->stream);
        if (rc != RAYZ_OK) return rc;
        if constexpr (to_u8) { // writePPM's transform before the gather: the tiles travel as u8, 4x smaller (src/image.zig:35-38)
            const size_t ne = (size_t)rayz_hip_shard_rows(&q) * row_elems;
            if (ne) {
                hipLaunchKernelGGL(tonemap_kernel, dim3((uint32_t)((ne + 255) / 256)), dim3(256), 0, ctx[i]->stream,
                                   (const float*)m->tile[i].get(), (uint8_t*)m->tile8[i].get(), ne);
                HIP_TRY(hipGetLastError());
            }
        }
    }
    // 2. one gather of the row tiles to the first device.  g0 .. g1 on the root's stream = from "the root's own rows are
    //    done" to "the frame is assembled": the transfer plus whatever the root waited for slower devices
    const auto wall0 = std::chrono::steady_clock::now();
    {
        DeviceScope scope(m->devices[0]);
        if (!m->g0) {
            HIP_TRY(m->g0.create());
            HIP_TRY(m->g1.create());
        }
        HIP_TRY(hipEventRecord(m->g0, ctx[0]->stream));
    }
    auto src = [&](uint32_t i) { return to_u8 ? m->tile8[i].get() : m->tile[i].get(); };
    if (m->transport == RAYZ_GATHER_RCCL) {
        NCCL_TRY(g_rccl.GroupStart());
        for (uint32_t i = 0; i < n; ++i) {
            ncclResult_t r = g_rccl.Gather(src(i), m->gathered, send_bytes, ncclUint8, 0, m->comms[i], ctx[i]->stream);
            if (r != ncclSuccess) {
                (void)g_rccl.GroupEnd();
                return fail(RAYZ_ERR_HIP, "ncclGather: %s", g_rccl.GetErrorString(r));
            }
        }
        NCCL_TRY(g_rccl.GroupEnd());
    } else { // peer copies, each on its source device's stream; the root's stream waits for all of them
        for (uint32_t i = 0; i < n; ++i) {
            DeviceScope scope(m->devices[i]);
            HIP_TRY(hipMemcpyPeerAsync(m->gathered.get() + (size_t)i * send_bytes, m->devices[0], src(i), m->devices[i], send_bytes,
                                       ctx[i]->stream));
            HIP_TRY(hipEventRecord(m->done[i], ctx[i]->stream));
        }
        DeviceScope scope(m->devices[0]);
        for (uint32_t i = 1; i < n; ++i) HIP_TRY(hipStreamWaitEvent(ctx[0]->stream, m->done[i], 0));
    }
    // 3. un-interleave on the root, copy out
    {
        DeviceScope scope(m->devices[0]);
        const size_t ne = (size_t)p->height * row_elems;
        hipLaunchKernelGGL(unshard_kernel<T>, dim3((uint32_t)((ne + 255) / 256)), dim3(256), 0, ctx[0]->stream,
                           (const T*)m->gathered.get(), (T*)m->frame.get(), p->height, (uint32_t)row_elems, q.tile_rows, n, max_rows);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(m->g1, ctx[0]->stream));
        HIP_TRY(hipMemcpyAsync(out, m->frame, frame_bytes, hipMemcpyDeviceToHost, ctx[0]->stream));
        HIP_TRY(hipStreamSynchronize(ctx[0]->stream));
        float gms = 0;
        HIP_TRY(hipEventElapsedTime(&gms, m->g0, m->g1));
        m->last_gather_ms = gms;
        m->last_frame_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - wall0).count();
    }
    // 4. counters: sums over the devices; kernel_ms is the slowest device's trace kernel
    RayzRenderStats tot{};
    m->last_dev.assign(n, RayzRenderStats{});
    for (uint32_t i = 0; i < n; ++i) {
        RayzRenderStats st{};
        rc = scene_sync(m->scenes[i].get(), &st);
        if (rc != RAYZ_OK) return rc;
        m->last_dev[i] = st;
        tot.primary_rays += st.primary_rays;
        tot.segments += st.segments;
        tot.sphere_tests += st.sphere_tests;
        tot.node_tests += st.node_tests;
        tot.kernel_ms = st.kernel_ms > tot.kernel_ms ? st.kernel_ms : tot.kernel_ms;
    }
    if (stats) *stats = tot;
    return RAYZ_OK;
}

template <class T>
int render_multi_oneshot(const int* devices, int n, const RayzSceneDesc* scene, const RayzCameraDesc* cam, const RayzRenderParams* p,
                         T* out, RayzRenderStats* stats) {
    RayzMulti* raw = nullptr;
    const int rc = multi_create(devices, n, scene, RAYZ_GATHER_RCCL, &raw);
    if (rc != RAYZ_OK) return rc;
    const std::unique_ptr<RayzMulti> m(raw);
    return multi_render<T>(m.get(), cam, p, out, stats);
}

// ---- ray queries (rayz_hip_scene_query*) ---------------------------------------------------------------
// query_key (rayz_device.hpp) and its inverse on the host: an order-preserving u64 of a double
unsigned long long query_key_host(double x) {
    unsigned long long b;
    std::memcpy(&b, &x, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
double query_unkey_host(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double x;
    std::memcpy(&x, &b, 8);
    return x;
}

// What every query entry checks before touching a device.
int check_query_args(RayzScene* s, uint32_t kind, uint32_t precision, uint32_t traversal, double tmin) {
    if (!s) return fail(RAYZ_ERR_BAD_ARG, "scene handle is null");
    if (kind > RAYZ_QUERY_ANY) return fail(RAYZ_ERR_BAD_ARG, "bad query kind %u", kind);
    if (precision > RAYZ_PRECISION_F64) return fail(RAYZ_ERR_BAD_ARG, "bad precision %u", precision);
    if (traversal > RAYZ_TRAVERSAL_AUTO) return fail(RAYZ_ERR_BAD_ARG, "bad traversal %u", traversal);
    if (!(tmin == tmin)) return fail(RAYZ_ERR_BAD_ARG, "tmin is NaN");
    return RAYZ_OK;
}

// The bound check of a batch: max |origin|, time range and refusals (query_bounds_kernel), read back — the one wait of a query.
constexpr uint32_t kQueryBoundBase = 32, kQueryCounterWords = kQueryBoundBase + 4 * kQueryBoundStride;
template <class R> int query_bounds(RayzScene* s, const DeviceCtx& ctx, const R* rays, uint32_t n, hipStream_t stream, double& S) {
    unsigned long long init[4 * kQueryBoundStride] = {};
    init[0] = query_key_host(0.0);
    init[kQueryBoundStride] = query_key_host(std::numeric_limits<double>::infinity());
    init[2 * kQueryBoundStride] = query_key_host(-std::numeric_limits<double>::infinity());
    unsigned long long* words = s->q_counters.get() + kQueryBoundBase;
    HIP_TRY(hipMemcpyAsync(words, init, sizeof(init), hipMemcpyHostToDevice, stream));
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)ctx.num_cu * 2, (n + 255) / 256));
    hipLaunchKernelGGL(query_bounds_kernel<R>, dim3(blocks), dim3(256), 0, stream, rays, n, words);
    HIP_TRY(hipGetLastError());
    unsigned long long got[4 * kQueryBoundStride] = {};
    HIP_TRY(hipMemcpyAsync(got, words, sizeof(got), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const unsigned long long flags = got[3 * kQueryBoundStride];
    if (flags & 1u) return fail(RAYZ_ERR_BAD_ARG, "query rays: a NaN or infinite origin, direction or time");
    if (flags & 8u) return fail(RAYZ_ERR_BAD_ARG, "query rays: an origin component beyond RAYZ_QUERY_MAX_ORIGIN (%g)", (double)RAYZ_QUERY_MAX_ORIGIN);
    if (flags & 2u) return fail(RAYZ_ERR_BAD_ARG, "query rays: a zero direction");
    if (flags & 16u)
        return fail(RAYZ_ERR_BAD_ARG, "query rays: a direction whose largest component lies outside [2^-32, 2^32] "
                                      "(RAYZ_QUERY_MIN_DIR, RAYZ_QUERY_MAX_DIR)");
    if (flags & 4u) return fail(RAYZ_ERR_BAD_ARG, "query rays: a NaN tmax");
    const double tlo = query_unkey_host(got[kQueryBoundStride]), thi = query_unkey_host(got[2 * kQueryBoundStride]);
    if (tlo < 0.0 || thi > 1.0)
        return fail(RAYZ_ERR_BAD_ARG, "query rays: time %g outside [0, 1] (the BVH's moving-sphere boxes cover [0, 1] only)",
                    tlo < 0.0 ? tlo : thi);
    S = query_unkey_host(got[0]) * (1.0 + 1e-6); // (the norm is rounded in f64: a relative margin far above its error)
    return RAYZ_OK;
}

// One query launch: rays (or the camera form when rays == NULL, `cam` / `p` then describe it) on the scene's device.
template <class R>
int query_impl(RayzScene* s, const DeviceCtx& ctx, uint32_t kind, uint32_t traversal, double tmin, uint32_t n, const R* rays,
               const RayzCameraDesc* cam, const RayzRenderParams* p, const RayzQueryOutputs* out, hipStream_t stream) {
    SceneBuffers<R>& b = buffers_of<R>(*s);
    if (s->last_stream && s->last_stream != stream) HIP_TRY(hipStreamSynchronize(s->last_stream)); // one launch in flight per scene
    if (!s->q_counters) {
        HIP_TRY(s->q_counters.alloc(kQueryCounterWords));
        HIP_TRY(hipMemset(s->q_counters, 0, kQueryCounterWords * sizeof(unsigned long long)));
    }
    if (!s->q_ev0) {
        HIP_TRY(s->q_ev0.create());
        HIP_TRY(s->q_ev1.create());
    }
    double S = 0;
    int rc = rays ? query_bounds<R>(s, ctx, rays, n, stream, S) : RAYZ_OK;
    if (rc != RAYZ_OK) return rc;
    if (!rays) S = camera_origin_bound(cam);
    bool use_bvh = false;
    rc = prepare_scene_bound<R>(s, b, S, traversal, stream, use_bvh);
    if (rc != RAYZ_OK) return rc;

    QueryArgs<R> A{};
    A.sc.stat = b.stat;
    A.sc.movy = b.movy;
    A.sc.movg = b.movg;
    A.sc.slot64 = s->narrow.slot64;
    A.sc.slot_pool = s->narrow.slot_pool;
    A.sc.sph_pool = b.sph_pool;
    A.sc.mat = b.mat;
    A.sc.tex = b.tex;
    A.sc.ns_pad = s->narrow.ns_pad;
    A.sc.ny_pad = s->narrow.ny_pad;
    A.sc.ng_pad = s->narrow.ng_pad;
    A.sc.n_spheres = (uint32_t)s->spheres.size();
    A.sc.tri = b.tri;
    A.sc.nt_pad = b.nt_pad;
    A.sc.n_triangles = (uint32_t)s->triangles.size();
    A.sc.bvh_nodes = (const f4*)b.bvh_nodes.get();
    for (int k = 0; k < 3; ++k) A.sc.bvh_glo[k] = b.grid.glo[k], A.sc.bvh_cell[k] = b.grid.cell[k];
    A.sc.bvh_leaf = b.bvh_leaf;
    A.sc.bvh_sph64 = s->narrow.bvh_sph64;
    A.sc.bvh_n_nodes = use_bvh ? b.bvh_n_inner : 0u;
    A.sc.bvh_leaf_stride = b.bvh_leaf_stride;
    A.sc.bvh_n_big_leaves = use_bvh ? b.n_big_leaves : 0u;
    for (int k = 0; k < 4; ++k) A.sc.bvh_big[k] = b.big_desc[k];
    A.sc.bvh_top = 0u;
    if (cam) fill_camera<R>(cam, A.cam);
    A.rays = rays;
    A.tmin = (R)tmin;
    A.n = n;
    A.kind = kind;
    if (!rays) {
        const uint32_t rows = rayz_hip_shard_rows(p);
        A.width = p->width;
        A.tile_rows = p->tile_rows ? p->tile_rows : RAYZ_DEFAULT_TILE_ROWS;
        A.shard_index = p->shard_index;
        A.shard_count = p->shard_count ? p->shard_count : 1u;
        A.tiled_pixels = p->width % 8 == 0 ? (uint32_t)((uint64_t)(rows / 8 * 8) * p->width) : 0u;
    }
    A.counters = s->q_counters;
    A.index = out->index;
    A.t = (R*)out->t;
    A.point = (R*)out->point;
    A.normal = (R*)out->normal;
    A.front = out->front_face;
    A.material = out->material;
    A.albedo = (R*)out->albedo;
    A.hit = out->hit;

    typedef void (*Kernel)(const QueryArgs<R>);
    Kernel kernel = query_kernel<R>;
    int block = 256, blocks_per_cu = 0;
    size_t lds = 0;
    if (use_bvh) {
        // the render's LDS layout (trace_window): top | stacks | oversized hittables' records, the top shortened should the
        // request be refused
        kernel = b.quantized ? query_kernel_bvh<R, true> : query_kernel_bvh<R, false>;
        block = (int)kBvhWg;
        const size_t stack_bytes = ((size_t)s->bvh_dev.depth + 3) * kBvhWg * sizeof(uint32_t);
        const size_t rec_bytes = b.quantized ? 32 : 64;
        uint32_t top_records = b.bvh_top;
        const int rc = request_lds(kernel, "query", block, rec_bytes, stack_bytes + (b.n_big_leaves ? kBvhBigLdsBytes : 0), top_records, lds, blocks_per_cu);
        if (rc != RAYZ_OK) return rc;
        const size_t top_bytes = (size_t)top_records * rec_bytes;
        A.bvh_top_words = (uint32_t)(top_bytes / sizeof(uint32_t));
        A.bvh_big_words = (uint32_t)((top_bytes + stack_bytes) / sizeof(uint32_t));
        A.sc.bvh_top = (uint32_t)top_bytes;
    }
    uint64_t grid = (n + (uint64_t)block - 1) / block;
    if (use_bvh) grid = std::min<uint64_t>(grid, (uint64_t)ctx.num_cu * std::max(1, blocks_per_cu));
    s->last_stream = stream;
    s->q_stream = stream;
    s->q_bvh = use_bvh;
    s->q_last = RayzRenderStats{};
    s->q_last.primary_rays = s->q_last.segments = n;
    HIP_TRY(hipMemsetAsync(s->q_counters, 0, 4 * sizeof(unsigned long long), stream));
    HIP_TRY(hipEventRecord(s->q_ev0, stream));
    hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(block), lds, stream, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->q_ev1, stream));
    s->queried = true;
    return RAYZ_OK;
}

template <class R>
int scene_query(RayzScene* s, const RayzQueryParams* q, const void* rays, const RayzQueryOutputs* out, void* stream_arg) {
    if (!q) return fail(RAYZ_ERR_BAD_ARG, "query params is null");
    DeviceCtx* ctx = nullptr;
    int rc = scene_ctx(s, &ctx);
    if (rc != RAYZ_OK) return rc;
    DeviceScope scope(s->device);
    const hipStream_t stream = stream_arg ? (hipStream_t)stream_arg : ctx->stream;
    return query_impl<R>(s, *ctx, q->kind, q->traversal, q->tmin, q->n_rays, (const R*)rays, nullptr, nullptr, out, stream);
}

template <class R>
int scene_query_camera(RayzScene* s, const RayzCameraDesc* cam, const RayzRenderParams* p, const RayzQueryOutputs* out,
                       void* stream_arg) {
    const uint32_t rows = rayz_hip_shard_rows(p);
    const uint64_t pixels = (uint64_t)rows * p->width;
    if (pixels >= (1ull << 31)) return fail(RAYZ_ERR_BAD_ARG, "camera query of %llu pixels", (unsigned long long)pixels);
    if (pixels == 0) return RAYZ_OK;
    DeviceCtx* ctx = nullptr;
    int rc = scene_ctx(s, &ctx);
    if (rc != RAYZ_OK) return rc;
    DeviceScope scope(s->device);
    const hipStream_t stream = stream_arg ? (hipStream_t)stream_arg : ctx->stream;
    return query_impl<R>(s, *ctx, RAYZ_QUERY_NEAREST, p->traversal, p->tmin, (uint32_t)pixels, nullptr, cam, p, out, stream);
}

int query_sync(RayzScene* s, RayzRenderStats* stats) {
    if (!s) return fail(RAYZ_ERR_BAD_ARG, "scene handle is null");
    if (!s->queried) {
        if (stats) *stats = s->q_last;
        return RAYZ_OK;
    }
    DeviceScope scope(s->device);
    HIP_TRY(hipStreamSynchronize(s->q_stream));
    unsigned long long c[32] = {};
    HIP_TRY(hipMemcpy(c, s->q_counters, sizeof(c), hipMemcpyDeviceToHost));
    if (s->q_bvh && c[31]) return fail(RAYZ_ERR_STATE, "query_kernel_bvh refused to run: its dynamic LDS segment does not start at LDS address 0");
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, s->q_ev0, s->q_ev1));
    s->q_last.sphere_tests = s->q_bvh ? c[3] : s->q_last.segments * (unsigned long long)(s->spheres.size() + s->triangles.size());
    s->q_last.node_tests = s->q_bvh ? c[2] : 0;
    s->q_last.kernel_ms = ms;
    s->queried = false;
    if (stats) *stats = s->q_last;
    return RAYZ_OK;
}

} // namespace

// ---- the à-trous denoiser (kernels: denoise.hpp) ----------------------------------------------------------------
struct RayzDenoiser {
    uint32_t magic = 0;
    int device = -1;
    uint32_t width = 0, height = 0;
    DevBuf<dn4> ga, gb, mod, col[2]; // n_pixels records each
    DevEvent ev[10];         // ev[0]: the run starts; ev[1]: packed; ev[2 + l]: level l done
    int last_ev = -1;        // the last event recorded, of a failed run too: what the next run and destroy wait for (-1: none yet)
    uint32_t levels_run = 0; // levels of the last COMPLETE run (0: none, or the last run failed half-way: no timing)
    ~RayzDenoiser() {
        if (last_ev >= 0) { // (waits on the handle's own event, never on the caller's stream, which may be gone by now)
            DeviceScope scope(device);
            (void)hipEventSynchronize(ev[last_ev]);
        }
        magic = 0;
    }
};

namespace {

constexpr uint32_t kDenoiserMagic = 0x444e5a52u;
constexpr uint32_t kDenoiseFlags = RAYZ_DENOISE_ALBEDO;

int denoiser_free(RayzDenoiser* dn) {
    if (!dn) return RAYZ_OK;
    if (dn->magic != kDenoiserMagic) return fail(RAYZ_ERR_STATE, "not a denoiser handle");
    delete dn;
    return RAYZ_OK;
}

int denoiser_create(int device, uint32_t width, uint32_t height, RayzDenoiser** out) {
    if (!out) return fail(RAYZ_ERR_BAD_ARG, "out handle pointer is null");
    *out = nullptr;
    if (!width || !height) return fail(RAYZ_ERR_BAD_ARG, "denoiser frame %ux%u: zero size", width, height);
    if ((uint64_t)width * height > RAYZ_DENOISE_MAX_PIXELS)
        return fail(RAYZ_ERR_BAD_ARG, "denoiser frame %ux%u: more than RAYZ_DENOISE_MAX_PIXELS pixels", width, height);
    {
        std::lock_guard<std::mutex> lock(g_mu);
        if (device < 0) {
            if (g_default < 0) return fail(RAYZ_ERR_NO_DEVICE, "rayz_hip_init has not succeeded");
            device = g_default;
        } else {
            const int rc = ensure_ctx(device);
            if (rc != RAYZ_OK) return rc;
        }
    }
    DeviceScope scope(device);
    auto dn = std::make_unique<RayzDenoiser>();
    dn->magic = kDenoiserMagic, dn->device = device, dn->width = width, dn->height = height;
    hipError_t e = hipSuccess;
    for (DevBuf<dn4>* b : {&dn->ga, &dn->gb, &dn->mod, &dn->col[0], &dn->col[1]})
        if (e == hipSuccess) e = b->alloc((size_t)width * height);
    for (DevEvent& ev : dn->ev)
        if (e == hipSuccess) e = ev.create();
    if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? RAYZ_ERR_OOM : RAYZ_ERR_HIP, "denoiser buffers: %s", hipGetErrorString(e));
    *out = dn.release();
    return RAYZ_OK;
}

// Every argument is checked before the handle, and nothing here touches a device until all of them passed.
int denoiser_run(RayzDenoiser* dn, const RayzDenoiseParams* params, const float* d_in, const RayzQueryOutputs* g, float* d_out,
                 void* stream_arg) {
    RayzDenoiseParams p{0, RAYZ_DENOISE_DEFAULT_NORMAL_POWER_LOG2, RAYZ_DENOISE_ALBEDO, 0, RAYZ_DENOISE_DEFAULT_SIGMA_COLOR,
                        RAYZ_DENOISE_DEFAULT_SIGMA_PLANE};
    if (params) p = *params;
    if (p.levels > 8) return fail(RAYZ_ERR_BAD_ARG, "denoise levels %u > 8", p.levels);
    if (p.normal_power_log2 > 16) return fail(RAYZ_ERR_BAD_ARG, "denoise normal_power_log2 %u > 16", p.normal_power_log2);
    if (p.flags & ~kDenoiseFlags) return fail(RAYZ_ERR_BAD_ARG, "unknown denoise flag bits 0x%x", p.flags & ~kDenoiseFlags);
    const float sc = (float)p.sigma_color, sp = (float)p.sigma_plane;
    const float sc2 = sc * sc, sp2 = sp * sp; // (what the kernels divide by: a sigma whose f32 square is 0 would divide 0 by 0)
    if (!(p.sigma_color > 0) || !(sc2 > 0)) return fail(RAYZ_ERR_BAD_ARG, "denoise sigma_color %g: must be positive (and its square in f32)", p.sigma_color);
    if (!(p.sigma_plane > 0) || !(sp2 > 0)) return fail(RAYZ_ERR_BAD_ARG, "denoise sigma_plane %g: must be positive (and its square in f32)", p.sigma_plane);
    if (!d_in || !d_out) return fail(RAYZ_ERR_BAD_ARG, "denoise: null colour buffer");
    if (!g) return fail(RAYZ_ERR_BAD_ARG, "denoise: null G-buffer");
    if (!g->index || !g->normal || !g->point) return fail(RAYZ_ERR_BAD_ARG, "denoise: the G-buffer needs index, normal and point");
    const bool demod = p.flags & RAYZ_DENOISE_ALBEDO;
    if (demod && !g->albedo) return fail(RAYZ_ERR_BAD_ARG, "denoise: RAYZ_DENOISE_ALBEDO needs the G-buffer's albedo");
    if (!dn || dn->magic != kDenoiserMagic) return fail(RAYZ_ERR_STATE, "not a denoiser handle");
    hipStream_t st = (hipStream_t)stream_arg;
    if (!st) {
        std::lock_guard<std::mutex> lock(g_mu);
        if (!g_ctx[dn->device].ok) return fail(RAYZ_ERR_NO_DEVICE, "device %d is not initialised (rayz_hip_init / shutdown order)", dn->device);
        st = g_ctx[dn->device].stream;
    }
    DeviceScope scope(dn->device);
    // one run in flight per handle: its buffers are reused, so this run's stream first waits (on the device) for the previous
    // run's last event — whichever stream that was on, and whether or not that stream still exists
    if (dn->last_ev >= 0) HIP_TRY(hipStreamWaitEvent(st, dn->ev[dn->last_ev], 0));
    const uint32_t levels = p.levels ? p.levels : RAYZ_DENOISE_DEFAULT_LEVELS;
    const size_t n = (size_t)dn->width * dn->height;
    dn->levels_run = 0; // (a run that fails half-way leaves no timing)
    HIP_TRY(hipEventRecord(dn->ev[0], st));
    dn->last_ev = 0;
    denoise_launch_pack(st, d_in, g->index, (const float*)g->normal, (const float*)g->point,
                        demod ? (const float*)g->albedo : nullptr, dn->ga, dn->gb, dn->mod, dn->col[0], n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(dn->ev[1], st));
    dn->last_ev = 1;
    DenoiseArgs a{};
    a.ga = dn->ga, a.gb = dn->gb, a.mod = dn->mod, a.rgb = d_out;
    a.width = dn->width, a.height = dn->height, a.normal_power_log2 = p.normal_power_log2, a.sp2 = sp2, a.sc2 = sc2;
    // which levels stage their taps in LDS: strides up to kDnLdsMaxStride (denoise.hpp) unless the measurement knob says otherwise
    const uint32_t lds_max = (uint32_t)tuning(RAYZ_DEBUG_DENOISE_LDS_STRIDE, kDnLdsMaxStride);
    for (uint32_t l = 0; l < levels; ++l) {
        a.src = dn->col[l & 1], a.dst = dn->col[(l & 1) ^ 1];
        a.stride = 1 << l, a.cl = (float)(1u << (2 * l));
        const bool lds = l <= (uint32_t)kDnMaxLdsLog2 && (1u << l) <= lds_max;
        if (l + 1 == levels) denoise_launch_level<true>(st, a, l, lds);
        else denoise_launch_level<false>(st, a, l, lds);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(dn->ev[2 + l], st));
        dn->last_ev = 2 + (int)l;
    }
    dn->levels_run = levels;
    return RAYZ_OK;
}

int denoiser_timing(RayzDenoiser* dn, uint32_t* levels, float* ms, uint32_t capacity) {
    if (!dn || dn->magic != kDenoiserMagic) return fail(RAYZ_ERR_STATE, "not a denoiser handle");
    if (!dn->levels_run) return fail(RAYZ_ERR_STATE, "no denoiser run to time");
    DeviceScope scope(dn->device);
    HIP_TRY(hipEventSynchronize(dn->ev[1 + dn->levels_run]));
    if (levels) *levels = dn->levels_run;
    for (uint32_t k = 0; ms && k < capacity && k <= dn->levels_run; ++k) HIP_TRY(hipEventElapsedTime(&ms[k], dn->ev[k], dn->ev[k + 1]));
    return RAYZ_OK;
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
        case RAYZ_DEBUG_BVHX: { // the retired kernels' knobs: checked in experiments/launch.hpp, refused by the product build
            const int rc = experiment_knob_check(knob, value);
            if (rc != RAYZ_OK) return rc;
            break;
        }
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

uint32_t rayz_hip_shard_rows(const RayzRenderParams* p) {
    if (!p) return 0;
    const uint32_t tr = p->tile_rows ? p->tile_rows : RAYZ_DEFAULT_TILE_ROWS, sc = p->shard_count ? p->shard_count : 1u;
    if (p->shard_index >= sc) return 0;
    uint32_t n = 0;
    for (uint32_t t = p->shard_index; (uint64_t)t * tr < p->height; t += sc) {
        const uint32_t r0 = t * tr;
        n += (p->height - r0 < tr) ? p->height - r0 : tr;
    }
    return n;
}

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
        {
            std::lock_guard<std::mutex> lock(g_mu);
            const int rc = ensure_ctx(device);
            if (rc != RAYZ_OK) return rc;
        }
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
        {
            std::lock_guard<std::mutex> lock(g_mu);
            device = g_default;
            if (device < 0) return fail(RAYZ_ERR_NO_DEVICE, "rayz_hip_init has not succeeded");
            own = g_ctx[device].stream;
        }
        if (!n_pixels) return (int)RAYZ_OK;
        if (!d_rgb || !d_rgb8) return fail(RAYZ_ERR_BAD_ARG, "null buffer");
        DeviceScope scope(device);
        const size_t n = n_pixels * 3;
        hipLaunchKernelGGL(tonemap_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream ? (hipStream_t)stream : own,
                           d_rgb, d_rgb8, n);
        HIP_TRY(hipGetLastError());
        return (int)RAYZ_OK;
    });
}

// ---- known answers: the kernel's device functions on caller inputs ---------------------------------------------
int rayz_hip_kat(uint32_t op, uint32_t precision, const double* in, uint32_t n, double* out) {
    return guarded([&] {
        if (op > RAYZ_KAT_SCAN_DISCS) return fail(RAYZ_ERR_BAD_ARG, "bad known-answer op %u", op);
        if (precision > RAYZ_PRECISION_F64) return fail(RAYZ_ERR_BAD_ARG, "bad precision %u", precision);
        if (!n) return (int)RAYZ_OK;
        if (!in || !out) return fail(RAYZ_ERR_BAD_ARG, "null buffer");
        int device;
        hipStream_t stream;
        {
            std::lock_guard<std::mutex> lock(g_mu);
            device = g_default;
            if (device < 0) return fail(RAYZ_ERR_NO_DEVICE, "rayz_hip_init has not succeeded");
            stream = g_ctx[device].stream;
        }
        std::vector<double> host(in, in + (size_t)n * RAYZ_KAT_IN_STRIDE);
        for (uint32_t i = 0; i < n; ++i) { // what the scene upload would have prepared for these hittables
            double* a = host.data() + (size_t)i * RAYZ_KAT_IN_STRIDE;
            // the list of uniforms must lie inside the record: the device reads u[0 .. n_u)
            if (op == RAYZ_KAT_GET_RAY || op == RAYZ_KAT_SCATTER) {
                const int at = op == RAYZ_KAT_GET_RAY ? 21 : 16;
                const double nu = a[at];
                const bool no_rng = op == RAYZ_KAT_GET_RAY && nu == -1.0; // getRay(px, py, null)
                if (!no_rng && !(nu >= 0 && nu <= RAYZ_KAT_IN_STRIDE - (at + 1) && nu == std::floor(nu)))
                    return fail(RAYZ_ERR_BAD_ARG, "record %u: n_u = %g is not an integer in [0, %d]%s", i, nu, RAYZ_KAT_IN_STRIDE - (at + 1),
                                op == RAYZ_KAT_GET_RAY ? " (or -1: no generator)" : "");
            }
            if (op == RAYZ_KAT_BOX_HIT) { // the box as a scene upload would hold it (S = this ray's origin, B = this box), in the format a[26] names
                rayz_bvh::Box bx;
                double B = 0;
                for (int k = 0; k < 3; ++k) bx.lo[k] = a[k], bx.hi[k] = a[3 + k], B = std::max({B, std::fabs(a[k]), std::fabs(a[3 + k])});
                if (a[26] != 0.0) { // f32 planes
                    const double pad = kBoxPadUlps * unit_roundoff<float>() * std::max(norm3(a + 6), B);
                    for (int k = 0; k < 3; ++k) {
                        a[14 + k] = (double)rayz_bvh::roundDown<float>(bx.lo[k] - pad), a[17 + k] = (double)rayz_bvh::roundUp<float>(bx.hi[k] + pad);
                        a[20 + k] = 0.0, a[23 + k] = 1.0;
                    }
                } else { // 16-bit plane indices on the grid over this box
                    double pad = kBoxPadUlps * unit_roundoff<float>() * (std::max(norm3(a + 6), B) + 2.0 * B);
                    const rayz_bvh::PlaneGrid g = rayz_bvh::PlaneGrid::over(bx.lo, bx.hi, 2.0 * pad);
                    pad = kBoxPadUlps * unit_roundoff<float>() * (std::max(norm3(a + 6), B) + g.extent);
                    uint32_t w[3];
                    g.quantize(bx, pad, w);
                    for (int k = 0; k < 3; ++k) a[14 + k] = w[k] & 0xffffu, a[17 + k] = w[k] >> 16, a[20 + k] = g.glo[k], a[23 + k] = g.cell[k];
                }
            }
            if (op == RAYZ_KAT_SCAN_DISCS) { // the padded squares the scan streams would hold for these four spheres
                const double cls = a[27];
                if (!(cls == 0.0 || cls == 1.0 || cls == 2.0 || cls == 3.0))
                    return fail(RAYZ_ERR_BAD_ARG, "record %u: class = %g is not 0, 1, 2 or 3", i, cls);
                if (!(a[32] == 0.0 || a[32] == 1.0)) return fail(RAYZ_ERR_BAD_ARG, "record %u: want_r2 = %g is not 0 or 1", i, a[32]);
                if (cls >= 2.0) { // a plane run: one f32 height, bit for bit (+0 and -0 are two runs), as plan_runs groups them
                    const uint32_t h = rayz_plane::bits32((float)a[4]);
                    for (int k = 1; k < 4; ++k)
                        if (rayz_plane::bits32((float)a[4 + k]) != h)
                            return fail(RAYZ_ERR_BAD_ARG, "record %u: plane-run class %g with cy[%d] = %.9g != cy[0] = %.9g in f32", i, cls, k,
                                        (double)(float)a[4 + k], (double)(float)a[4]);
                }
                double S = norm3(a + 20);
                RayzSphere q[4] = {};
                for (int k = 0; k < 4; ++k) {
                    q[k].center[0] = a[k], q[k].center[1] = a[4 + k], q[k].center[2] = a[8 + k];
                    q[k].radius = a[12 + k];
                    q[k].velocity[1] = cls == 1.0 || cls == 3.0 ? a[16 + k] : 0.0;
                    S = std::max(S, norm3(q[k].center) + norm3(q[k].velocity) + std::fabs(q[k].radius));
                }
                for (int k = 0; k < 4; ++k)
                    a[28 + k] = precision == RAYZ_PRECISION_F32 ? (double)pad_radius2_scan<float>(q[k], S) : (double)pad_radius2_scan<double>(q[k], S);
            }
            if (op == RAYZ_KAT_SPHERE_HIT) {
                RayzSphere q{};
                for (int k = 0; k < 3; ++k) q.center[k] = a[k], q.velocity[k] = a[3 + k];
                q.radius = a[6];
                const double S = std::max(norm3(a + 7), norm3(q.center) + norm3(q.velocity) + std::fabs(q.radius));
                a[16] = precision == RAYZ_PRECISION_F32 ? (double)pad_radius2_scan<float>(q, S) : (double)pad_radius2_scan<double>(q, S);
            }
        }
        DeviceScope scope(device);
        DevBuf<double> d_in, d_out;
        const size_t in_bytes = host.size() * sizeof(double), out_bytes = (size_t)n * RAYZ_KAT_OUT_STRIDE * sizeof(double);
        hipError_t e = d_in.alloc(host.size());
        if (e == hipSuccess) e = d_out.alloc((size_t)n * RAYZ_KAT_OUT_STRIDE);
        if (e == hipSuccess) e = hipMemcpyAsync(d_in, host.data(), in_bytes, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) {
            if (precision == RAYZ_PRECISION_F32) hipLaunchKernelGGL(kat_kernel<float>, dim3((n + 63) / 64), dim3(64), 0, stream, op, d_in.get(), n, d_out.get());
            else hipLaunchKernelGGL(kat_kernel<double>, dim3((n + 63) / 64), dim3(64), 0, stream, op, d_in.get(), n, d_out.get());
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? RAYZ_ERR_OOM : RAYZ_ERR_HIP, "rayz_hip_kat: %s", hipGetErrorString(e));
        return (int)RAYZ_OK;
    });
}

// ---- several devices behind one call ----------------------------------------------------------------------
int rayz_hip_multi_create(const int* devices, int n_devices, const RayzSceneDesc* scene, uint32_t transport, RayzMulti** out) {
    return guarded([&] { return multi_create(devices, n_devices, scene, transport, out); });
}

int rayz_hip_multi_destroy(RayzMulti* m) {
    return guarded([&] { return multi_free(m); });
}

int rayz_hip_multi_info(const RayzMulti* m, int* n_devices, uint32_t* transport, int* rccl_version) {
    if (!m) return fail(RAYZ_ERR_STATE, "multi handle is null");
    if (n_devices) *n_devices = (int)m->devices.size();
    if (transport) *transport = m->transport;
    if (rccl_version) *rccl_version = m->rccl_version;
    return RAYZ_OK;
}

int rayz_hip_multi_device_stats(const RayzMulti* m, int index, RayzRenderStats* stats) {
    if (!m) return fail(RAYZ_ERR_STATE, "multi handle is null");
    if (!stats) return fail(RAYZ_ERR_BAD_ARG, "stats pointer is null");
    if (index < 0 || (size_t)index >= m->devices.size()) return fail(RAYZ_ERR_BAD_ARG, "device index %d out of range", index);
    if (m->last_dev.size() != m->devices.size()) return fail(RAYZ_ERR_STATE, "no frame has been rendered on this handle");
    *stats = m->last_dev[(size_t)index];
    return RAYZ_OK;
}

int rayz_hip_multi_timing(const RayzMulti* m, double* gather_ms, double* frame_ms) {
    if (!m) return fail(RAYZ_ERR_STATE, "multi handle is null");
    if (m->last_dev.size() != m->devices.size()) return fail(RAYZ_ERR_STATE, "no frame has been rendered on this handle");
    if (gather_ms) *gather_ms = m->last_gather_ms;
    if (frame_ms) *frame_ms = m->last_frame_ms;
    return RAYZ_OK;
}

int rayz_hip_multi_render(RayzMulti* m, const RayzCameraDesc* cam, const RayzRenderParams* p, float* rgb_out, RayzRenderStats* stats) {
    return guarded([&] { return multi_render<float>(m, cam, p, rgb_out, stats); });
}
int rayz_hip_multi_render_f64(RayzMulti* m, const RayzCameraDesc* cam, const RayzRenderParams* p, double* rgb_out,
                              RayzRenderStats* stats) {
    return guarded([&] { return multi_render<double>(m, cam, p, rgb_out, stats); });
}
int rayz_hip_multi_render_u8(RayzMulti* m, const RayzCameraDesc* cam, const RayzRenderParams* p, uint8_t* rgb8_out,
                             RayzRenderStats* stats) {
    return guarded([&] { return multi_render<uint8_t>(m, cam, p, rgb8_out, stats); });
}

int rayz_hip_render_multi(const int* devices, int n_devices, const RayzSceneDesc* scene, const RayzCameraDesc* cam,
                          const RayzRenderParams* p, float* rgb_out, RayzRenderStats* stats) {
    return guarded([&] { return render_multi_oneshot<float>(devices, n_devices, scene, cam, p, rgb_out, stats); });
}
int rayz_hip_render_multi_f64(const int* devices, int n_devices, const RayzSceneDesc* scene, const RayzCameraDesc* cam,
                              const RayzRenderParams* p, double* rgb_out, RayzRenderStats* stats) {
    return guarded([&] { return render_multi_oneshot<double>(devices, n_devices, scene, cam, p, rgb_out, stats); });
}

// src/renderer.zig:80-97 (the loop nest) in passes, with src/renderer.zig:84,98-99's progress report in reach of the caller
int rayz_hip_progressive_create(RayzScene* scene, const RayzCameraDesc* camera, const RayzRenderParams* params,
                                RayzProgressive** out) {
    return guarded([&] { return progressive_create(scene, camera, params, out); });
}

int rayz_hip_progressive_step(RayzProgressive* pr, uint32_t min_samples, float* d_preview, void* stream) {
    return guarded([&] { return progressive_step<float>(pr, min_samples, d_preview, stream, RAYZ_PRECISION_F32); });
}

int rayz_hip_progressive_step_f64(RayzProgressive* pr, uint32_t min_samples, double* d_preview, void* stream) {
    return guarded([&] { return progressive_step<double>(pr, min_samples, d_preview, stream, RAYZ_PRECISION_F64); });
}

int rayz_hip_progressive_info(const RayzProgressive* pr, uint32_t* samples_done, uint32_t* chunks_done, uint32_t* n_chunks,
                              RayzRenderStats* total) {
    return guarded([&] { return progressive_info(pr, samples_done, chunks_done, n_chunks, total); });
}

int rayz_hip_progressive_track_noise(RayzProgressive* pr) {
    return guarded([&] { return progressive_track_noise(pr); });
}

int rayz_hip_progressive_noise(RayzProgressive* pr, const RayzNoiseParams* p, float* d_var, float* d_rel2, RayzNoiseSummary* summary,
                               void* stream) {
    return guarded([&] { return progressive_noise(pr, p, d_var, d_rel2, summary, stream); });
}

int rayz_hip_progressive_noise_state(RayzProgressive* pr, double* d_q, void* stream) {
    return guarded([&] { return progressive_noise_state(pr, d_q, stream); });
}

int rayz_hip_progressive_run_until(RayzProgressive* pr, const RayzNoiseParams* p, double max_unconverged_fraction,
                                   uint32_t min_samples_per_pass, float* d_preview, RayzNoiseSummary* last, void* stream) {
    return guarded([&] {
        return progressive_run_until<float>(pr, p, max_unconverged_fraction, min_samples_per_pass, d_preview, last, stream, RAYZ_PRECISION_F32);
    });
}

int rayz_hip_progressive_run_until_f64(RayzProgressive* pr, const RayzNoiseParams* p, double max_unconverged_fraction,
                                       uint32_t min_samples_per_pass, double* d_preview, RayzNoiseSummary* last, void* stream) {
    return guarded([&] {
        return progressive_run_until<double>(pr, p, max_unconverged_fraction, min_samples_per_pass, d_preview, last, stream, RAYZ_PRECISION_F64);
    });
}

int rayz_hip_noise_kat(uint32_t precision, const double* chunk_sums, const uint32_t* chunk_sizes, uint32_t n_pixels, uint32_t n_chunks,
                       const RayzNoiseParams* p, double* q_out, double* var_out, double* rel2_out, RayzNoiseSummary* summary) {
    return guarded([&] { return noise_kat(precision, chunk_sums, chunk_sizes, n_pixels, n_chunks, p, q_out, var_out, rel2_out, summary); });
}

int rayz_hip_progressive_destroy(RayzProgressive* pr) {
    return guarded([&] { return progressive_free(pr); });
}

int rayz_hip_scene_query(RayzScene* s, const RayzQueryParams* q, const void* d_rays, const RayzQueryOutputs* out, void* stream) {
    // every argument is checked before the first HIP call
    if (!q) return fail(RAYZ_ERR_BAD_ARG, "query params is null");
    int rc = check_query_args(s, q->kind, q->precision, q->traversal, q->tmin);
    if (rc != RAYZ_OK) return rc;
    if (!out) return fail(RAYZ_ERR_BAD_ARG, "outputs is null");
    if (q->n_rays == 0) return RAYZ_OK;
    if (!d_rays) return fail(RAYZ_ERR_BAD_ARG, "rays is null");
    return guarded([&] {
        return q->precision == RAYZ_PRECISION_F64 ? scene_query<double>(s, q, d_rays, out, stream)
                                                  : scene_query<float>(s, q, d_rays, out, stream);
    });
}

int rayz_hip_scene_query_camera(RayzScene* s, const RayzCameraDesc* cam, const RayzRenderParams* p, const RayzQueryOutputs* out,
                                void* stream) {
    if (!p) return fail(RAYZ_ERR_BAD_ARG, "params is null");
    int rc = check_query_args(s, RAYZ_QUERY_NEAREST, p->precision, p->traversal, p->tmin);
    if (rc != RAYZ_OK) return rc;
    if (!cam) return fail(RAYZ_ERR_BAD_ARG, "camera is null");
    if (!out) return fail(RAYZ_ERR_BAD_ARG, "outputs is null");
    if (!p->width || !p->height) return fail(RAYZ_ERR_BAD_ARG, "width and height must be > 0");
    const uint32_t sc = p->shard_count ? p->shard_count : 1;
    if (p->shard_index >= sc) return fail(RAYZ_ERR_BAD_ARG, "shard_index %u >= shard_count %u", p->shard_index, sc);
    return guarded([&] {
        return p->precision == RAYZ_PRECISION_F64 ? scene_query_camera<double>(s, cam, p, out, stream)
                                                  : scene_query_camera<float>(s, cam, p, out, stream);
    });
}

int rayz_hip_query_sync(RayzScene* s, RayzRenderStats* stats) {
    return guarded([&] { return query_sync(s, stats); });
}

int rayz_hip_denoiser_create(int device, uint32_t width, uint32_t height, RayzDenoiser** out) {
    return guarded([&] { return denoiser_create(device, width, height, out); });
}

int rayz_hip_denoiser_run(RayzDenoiser* dn, const RayzDenoiseParams* params, const float* d_rgb_in, const RayzQueryOutputs* gbuffer,
                          float* d_rgb_out, void* hip_stream) {
    return guarded([&] { return denoiser_run(dn, params, d_rgb_in, gbuffer, d_rgb_out, hip_stream); });
}

int rayz_hip_denoiser_timing(RayzDenoiser* dn, uint32_t* levels_or_null, float* ms_or_null, uint32_t capacity) {
    return guarded([&] { return denoiser_timing(dn, levels_or_null, ms_or_null, capacity); });
}

int rayz_hip_denoiser_destroy(RayzDenoiser* dn) {
    return guarded([&] { return denoiser_free(dn); });
}

} // extern "C"
