// frame_handle.hpp — what the handles of the whole-frame filters share (denoiser.hpp, temporal.hpp): per-pixel record buffers of one
// frame size on one device, events of the handle's own, and the rule that one run is in flight per handle.
// Included by rayz_hip.hip after host_base.hpp.  A handle type H derives from FrameHandle and names itself: H::kMagic, and H::kNoun
// for the messages ("denoiser", "temporal").
#pragma once

template <int N_BUFS, int N_EVENTS> struct FrameHandle {
    uint32_t magic = 0;
    int device = -1;
    uint32_t width = 0, height = 0;
    DevBuf<dn4> buf[N_BUFS]; // width x height records each
    DevEvent ev[N_EVENTS];
    int last_ev = -1;        // the last event recorded, of a failed run too: what the next run and destroy wait for (-1: none yet)
    ~FrameHandle() {
        if (last_ev >= 0) { // (waits on the handle's own event, never on the caller's stream, which may be gone by now)
            DeviceScope scope(device);
            (void)hipEventSynchronize(ev[last_ev]);
        }
        magic = 0;
    }
};

namespace {

template <class H> int frame_handle_check(const H* h) {
    if (!h || h->magic != H::kMagic) return fail(RAYZ_ERR_STATE, "not a %s handle", H::kNoun);
    return RAYZ_OK;
}

template <class H> int frame_handle_free(H* h) {
    if (!h) return RAYZ_OK;
    RAYZ_TRY(frame_handle_check(h));
    delete h;
    return RAYZ_OK;
}

template <class H> int frame_handle_create(int device, uint32_t width, uint32_t height, H** out) {
    if (!out) return fail(RAYZ_ERR_BAD_ARG, "out handle pointer is null");
    *out = nullptr;
    if (!width || !height) return fail(RAYZ_ERR_BAD_ARG, "%s frame %ux%u: zero size", H::kNoun, width, height);
    if ((uint64_t)width * height > RAYZ_DENOISE_MAX_PIXELS)
        return fail(RAYZ_ERR_BAD_ARG, "%s frame %ux%u: more than RAYZ_DENOISE_MAX_PIXELS pixels", H::kNoun, width, height);
    if (device < 0) {
        hipStream_t unused;
        RAYZ_TRY(default_device(device, unused));
    } else RAYZ_TRY(ensure_ctx_locked(device));
    DeviceScope scope(device);
    auto h = std::make_unique<H>();
    h->magic = H::kMagic, h->device = device, h->width = width, h->height = height;
    hipError_t e = hipSuccess;
    for (DevBuf<dn4>& b : h->buf)
        if (e == hipSuccess) e = b.alloc((size_t)width * height);
    for (DevEvent& ev : h->ev)
        if (e == hipSuccess) e = ev.create();
    if (e != hipSuccess) {
        char what[32];
        snprintf(what, sizeof(what), "%s buffers", H::kNoun);
        return hip_fail(e, what);
    }
    *out = h.release();
    return RAYZ_OK;
}

// The guides every frame filter needs, `who` being the message's subject ("denoise", "temporal").
int frame_gbuffer_check(const char* who, const RayzQueryOutputs* g) {
    if (!g) return fail(RAYZ_ERR_BAD_ARG, "%s: null G-buffer", who);
    if (!g->index || !g->normal || !g->point) return fail(RAYZ_ERR_BAD_ARG, "%s: the G-buffer needs index, normal and point", who);
    return RAYZ_OK;
}

// The stream a run works on: the caller's, taken as it is, or else the device's own stream, which has to exist then.
template <class H> int frame_handle_stream(const H* h, void* stream_arg, hipStream_t& st) {
    st = stream_or(stream_arg, nullptr);
    if (st) return RAYZ_OK;
    std::lock_guard<std::mutex> lock(g_mu);
    if (!g_ctx[h->device].ok) return fail(RAYZ_ERR_NO_DEVICE, "device %d is not initialised (rayz_hip_init / shutdown order)", h->device);
    st = g_ctx[h->device].stream;
    return RAYZ_OK;
}

// One run in flight per handle: its buffers are reused (or read back) by the next, so a run's stream first waits (on the device) for
// the previous run's last event — whichever stream that was on, and whether or not that stream still exists.
template <class H> int frame_handle_wait_previous(const H* h, hipStream_t st) {
    if (h->last_ev >= 0) HIP_TRY(hipStreamWaitEvent(st, h->ev[h->last_ev], 0));
    return RAYZ_OK;
}

// Records the handle's event k on the run's stream and remembers it ..
template <class H> int frame_handle_record(H* h, int k, hipStream_t st) {
    HIP_TRY(hipEventRecord(h->ev[k], st));
    h->last_ev = k;
    return RAYZ_OK;
}
// .. behind a launch, which is checked first.
template <class H> int frame_handle_launched(H* h, int k, hipStream_t st) {
    HIP_TRY(hipGetLastError());
    return frame_handle_record(h, k, st);
}

} // namespace
