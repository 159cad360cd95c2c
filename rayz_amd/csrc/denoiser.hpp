// denoiser.hpp — the à-trous denoiser's handle (rayz_hip_denoiser_*, DESIGN.md §4.11, the variance-guided mode §4.13; kernels and
// their launches: denoise.hpp).
// Included by rayz_hip.hip; of the renderer it needs the device contexts only.
#pragma once

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
    if (device < 0) {
        hipStream_t unused;
        RAYZ_TRY(default_device(device, unused));
    } else RAYZ_TRY(ensure_ctx_locked(device));
    DeviceScope scope(device);
    auto dn = std::make_unique<RayzDenoiser>();
    dn->magic = kDenoiserMagic, dn->device = device, dn->width = width, dn->height = height;
    hipError_t e = hipSuccess;
    for (DevBuf<dn4>* b : {&dn->ga, &dn->gb, &dn->mod, &dn->col[0], &dn->col[1]})
        if (e == hipSuccess) e = b->alloc((size_t)width * height);
    for (DevEvent& ev : dn->ev)
        if (e == hipSuccess) e = ev.create();
    if (e != hipSuccess) return hip_fail(e, "denoiser buffers");
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
    hipStream_t st = stream_or(stream_arg, nullptr);
    if (!st) { // (the device's own stream, which has to exist then; a caller's stream is taken as it is)
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

// The variance-guided mode (§4.13): denoiser_run's checks, order and events with the guided kernels; the handle's buffers serve
// either mode (the colour records' .w slot carries the variance here and 0 there), so the modes may alternate on one handle.
int denoiser_run_guided(RayzDenoiser* dn, const RayzDenoiseGuidedParams* params, const float* d_in, const float* d_var_rgb,
                        const RayzQueryOutputs* g, float* d_out, float* d_var_out, void* stream_arg) {
    RayzDenoiseGuidedParams p{0, RAYZ_DENOISE_DEFAULT_NORMAL_POWER_LOG2, RAYZ_DENOISE_ALBEDO, 0, RAYZ_DENOISE_GUIDED_DEFAULT_SIGMA_COLOR,
                              RAYZ_DENOISE_DEFAULT_SIGMA_PLANE, RAYZ_DENOISE_GUIDED_DEFAULT_VAR_FLOOR};
    if (params) p = *params;
    if (p.levels > 8) return fail(RAYZ_ERR_BAD_ARG, "denoise levels %u > 8", p.levels);
    if (p.normal_power_log2 > 16) return fail(RAYZ_ERR_BAD_ARG, "denoise normal_power_log2 %u > 16", p.normal_power_log2);
    if (p.flags & ~kDenoiseFlags) return fail(RAYZ_ERR_BAD_ARG, "unknown denoise flag bits 0x%x", p.flags & ~kDenoiseFlags);
    const float sc = (float)p.sigma_color, sp = (float)p.sigma_plane, vf = (float)p.var_floor;
    const float sc2 = sc * sc, sp2 = sp * sp;
    if (!(p.sigma_color > 0) || !(sc2 > 0)) return fail(RAYZ_ERR_BAD_ARG, "denoise sigma_color %g: must be positive (and its square in f32)", p.sigma_color);
    if (!(p.sigma_plane > 0) || !(sp2 > 0)) return fail(RAYZ_ERR_BAD_ARG, "denoise sigma_plane %g: must be positive (and its square in f32)", p.sigma_plane);
    // (den = sc2·(gv + vf) >= sc2·vf is what a tap divides by: were it 0, the centre tap would divide 0 by 0)
    if (!(p.var_floor > 0) || !(sc2 * vf > 0))
        return fail(RAYZ_ERR_BAD_ARG, "denoise var_floor %g: must be positive (and sigma_color^2 x var_floor in f32)", p.var_floor);
    if (!d_in || !d_out) return fail(RAYZ_ERR_BAD_ARG, "denoise: null colour buffer");
    if (!d_var_rgb) return fail(RAYZ_ERR_BAD_ARG, "denoise: the guided mode needs the per-channel variance (rayz_hip_progressive_noise_rgb)");
    if (!g) return fail(RAYZ_ERR_BAD_ARG, "denoise: null G-buffer");
    if (!g->index || !g->normal || !g->point) return fail(RAYZ_ERR_BAD_ARG, "denoise: the G-buffer needs index, normal and point");
    const bool demod = p.flags & RAYZ_DENOISE_ALBEDO;
    if (demod && !g->albedo) return fail(RAYZ_ERR_BAD_ARG, "denoise: RAYZ_DENOISE_ALBEDO needs the G-buffer's albedo");
    if (!dn || dn->magic != kDenoiserMagic) return fail(RAYZ_ERR_STATE, "not a denoiser handle");
    hipStream_t st = stream_or(stream_arg, nullptr);
    if (!st) {
        std::lock_guard<std::mutex> lock(g_mu);
        if (!g_ctx[dn->device].ok) return fail(RAYZ_ERR_NO_DEVICE, "device %d is not initialised (rayz_hip_init / shutdown order)", dn->device);
        st = g_ctx[dn->device].stream;
    }
    DeviceScope scope(dn->device);
    if (dn->last_ev >= 0) HIP_TRY(hipStreamWaitEvent(st, dn->ev[dn->last_ev], 0)); // one run in flight per handle, of either mode
    const uint32_t levels = p.levels ? p.levels : RAYZ_DENOISE_GUIDED_DEFAULT_LEVELS;
    const size_t n = (size_t)dn->width * dn->height;
    dn->levels_run = 0;
    HIP_TRY(hipEventRecord(dn->ev[0], st));
    dn->last_ev = 0;
    denoise_launch_pack_guided(st, d_in, d_var_rgb, g->index, (const float*)g->normal, (const float*)g->point,
                               demod ? (const float*)g->albedo : nullptr, dn->ga, dn->gb, dn->mod, dn->col[0], n);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(dn->ev[1], st));
    dn->last_ev = 1;
    DenoiseGuidedArgs a{};
    a.ga = dn->ga, a.gb = dn->gb, a.mod = dn->mod, a.rgb = d_out, a.var = d_var_out;
    a.width = dn->width, a.height = dn->height, a.normal_power_log2 = p.normal_power_log2, a.sp2 = sp2, a.sc2 = sc2, a.vf = vf;
    const uint32_t lds_max = (uint32_t)tuning(RAYZ_DEBUG_DENOISE_LDS_STRIDE, kDnLdsMaxStride);
    for (uint32_t l = 0; l < levels; ++l) {
        a.src = dn->col[l & 1], a.dst = dn->col[(l & 1) ^ 1];
        a.stride = 1 << l;
        const bool lds = l <= (uint32_t)kDnMaxLdsLog2 && (1u << l) <= lds_max;
        if (l + 1 == levels) denoise_launch_level_guided<true>(st, a, l, lds);
        else denoise_launch_level_guided<false>(st, a, l, lds);
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

int rayz_hip_denoiser_create(int device, uint32_t width, uint32_t height, RayzDenoiser** out) {
    return guarded([&] { return denoiser_create(device, width, height, out); });
}

int rayz_hip_denoiser_run(RayzDenoiser* dn, const RayzDenoiseParams* params, const float* d_rgb_in, const RayzQueryOutputs* gbuffer,
                          float* d_rgb_out, void* hip_stream) {
    return guarded([&] { return denoiser_run(dn, params, d_rgb_in, gbuffer, d_rgb_out, hip_stream); });
}

int rayz_hip_denoiser_run_guided(RayzDenoiser* dn, const RayzDenoiseGuidedParams* params, const float* d_rgb_in, const float* d_var_rgb,
                                 const RayzQueryOutputs* gbuffer, float* d_rgb_out, float* d_var_out_or_null, void* hip_stream) {
    return guarded([&] { return denoiser_run_guided(dn, params, d_rgb_in, d_var_rgb, gbuffer, d_rgb_out, d_var_out_or_null, hip_stream); });
}

int rayz_hip_denoiser_timing(RayzDenoiser* dn, uint32_t* levels_or_null, float* ms_or_null, uint32_t capacity) {
    return guarded([&] { return denoiser_timing(dn, levels_or_null, ms_or_null, capacity); });
}

int rayz_hip_denoiser_destroy(RayzDenoiser* dn) {
    return guarded([&] { return denoiser_free(dn); });
}

} // extern "C"
