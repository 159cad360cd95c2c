// multi_device.hpp — several devices behind one call (rayz_hip_multi_*, rayz_hip_render_multi*): one scene and one stream per device, one
// host thread, one gather of the row tiles to the first device (RCCL or peer copies).  Included by rayz_hip.hip, behind render_impl.
#pragma once

#include <rccl/rccl.h> // types and prototypes only: the library is opened with dlopen at the first multi-device call
#include <dlfcn.h>
#include <chrono>

namespace {

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
    RAYZ_TRY(check_device_list(devices, n_devices, dup_ok));
    RAYZ_TRY(validate_scene(scene));
    {
        std::lock_guard<std::mutex> lock(g_mu);
        for (int i = 0; i < n_devices; ++i) RAYZ_TRY(ensure_ctx(devices[i]));
        if (transport == RAYZ_GATHER_RCCL) RAYZ_TRY(rccl_load());
    }
    auto m = std::make_unique<RayzMulti>(devices, n_devices);
    m->transport = transport;
    for (int i = 0; i < n_devices; ++i) RAYZ_TRY(scene_new(scene, devices[i], m->scenes[i]));
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
    RAYZ_TRY(validate_params(p));
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
        RAYZ_TRY(scene_ctx(m->scenes[i]->device, &ctx[i]));
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
        RAYZ_TRY(render_impl<R>(m->scenes[i].get(), *ctx[i], buffers_of<R>(*m->scenes[i]), cam, &q, (R*)m->tile[i].get(), ctx[i]->stream));
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
        RAYZ_TRY(scene_sync(m->scenes[i].get(), &st));
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
    RAYZ_TRY(multi_create(devices, n, scene, RAYZ_GATHER_RCCL, &raw));
    const std::unique_ptr<RayzMulti> m(raw);
    return multi_render<T>(m.get(), cam, p, out, stats);
}

} // namespace

extern "C" {

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

} // extern "C"
