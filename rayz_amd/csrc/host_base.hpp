// host_base.hpp — what every part of the host library (rayz_hip.hip and the feature headers it includes) stands on: the error
// string and the error macros, the per-device contexts, the measurement knobs, and the owners of device memory and events.
#pragma once
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

// A failed HIP call as this library's return code and message: `what` failed (at file:line, where HIP_TRY names the call itself).
int hip_fail(hipError_t e, const char* what, const char* file = nullptr, int line = 0) {
    const int code = e == hipErrorOutOfMemory ? RAYZ_ERR_OOM : RAYZ_ERR_HIP;
    return file ? fail(code, "%s: %s (%s:%d)", what, hipGetErrorString(e), file, line) : fail(code, "%s: %s", what, hipGetErrorString(e));
}

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return hip_fail(e_, #expr, __FILE__, __LINE__); } while (0)
// .. and a call of this library's own: its failure (message set by whoever failed) is the caller's.
#define RAYZ_TRY(expr) do { const int rc_ = (expr); if (rc_ != RAYZ_OK) return rc_; } while (0)

// ---- which device, which stream (none of these waits for anything or selects a device: DeviceScope stays visible at each site) ----
// The context a scene renders on, `device` being RayzScene::device.  A scene created without a device is bound to the default here.
int scene_ctx(int& device, DeviceCtx** out) {
    std::lock_guard<std::mutex> lock(g_mu);
    if (device < 0) {
        if (g_default < 0) return fail(RAYZ_ERR_NO_DEVICE, "rayz_hip_init has not succeeded");
        device = g_default;
    }
    if (!g_ctx[device].ok) return fail(RAYZ_ERR_NO_DEVICE, "device %d is not initialised (rayz_hip_init / shutdown order)", device);
    *out = &g_ctx[device];
    return RAYZ_OK;
}

// The stream an entry point works on: the caller's (a hipStream_t passed as void*), or `own` when the caller passed none.
hipStream_t stream_or(void* stream_arg, hipStream_t own) { return stream_arg ? (hipStream_t)stream_arg : own; }

// .. both for an entry point that takes a scene and a stream.
int scene_stream(int& device, void* stream_arg, DeviceCtx*& ctx, hipStream_t& stream) {
    RAYZ_TRY(scene_ctx(device, &ctx));
    stream = stream_or(stream_arg, ctx->stream);
    return RAYZ_OK;
}

// The default device (the last successful rayz_hip_init's: what entry points without a device argument use) with its stream, or
// -1 while there is none; default_device fails then.
int default_device_or_none(hipStream_t* stream = nullptr) {
    std::lock_guard<std::mutex> lock(g_mu);
    if (g_default >= 0 && stream) *stream = g_ctx[g_default].stream;
    return g_default;
}
int default_device(int& device, hipStream_t& stream) {
    device = default_device_or_none(&stream);
    return device < 0 ? fail(RAYZ_ERR_NO_DEVICE, "rayz_hip_init has not succeeded") : (int)RAYZ_OK;
}

} // namespace
