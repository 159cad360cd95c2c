// denoiser.hpp — the à-trous denoiser's handle (rayz_hip_denoiser_*, DESIGN.md §4.11, the variance-guided mode §4.13; kernels and
// their launches: denoise.hpp; what it shares with the temporal handle: frame_handle.hpp).
// Included by rayz_hip.hip; of the renderer it needs the device contexts only.
#pragma once

// buf: ga, gb, mod, col[2] (the colour records' .w slot carries the variance in the guided mode and 0 in the plain one, so the modes
// may alternate on one handle).  ev[0]: the run starts; ev[1]: packed; ev[2 + l]: level l done.
struct RayzDenoiser : FrameHandle<5, 10> {
    static constexpr uint32_t kMagic = 0x444e5a52u;
    static constexpr const char* kNoun = "denoiser";
    uint32_t levels_run = 0; // levels of the last COMPLETE run (0: none, or the last run failed half-way: no timing)
    const uint32_t* keys = nullptr; // the caller's surface keys (rayz_hip_denoiser_set_keys), read by every run's pack pass; NULL: none
};

namespace {

constexpr uint32_t kDenoiseFlags = RAYZ_DENOISE_ALBEDO;

// The parameters of a run of either mode as the guided mode's (the plain mode has no var_floor); NULL: the mode's defaults.
RayzDenoiseGuidedParams denoise_params(const RayzDenoiseParams* p) {
    if (!p) return {0, RAYZ_DENOISE_DEFAULT_NORMAL_POWER_LOG2, RAYZ_DENOISE_ALBEDO, 0, RAYZ_DENOISE_DEFAULT_SIGMA_COLOR, RAYZ_DENOISE_DEFAULT_SIGMA_PLANE, 0};
    return {p->levels, p->normal_power_log2, p->flags, p->_pad, p->sigma_color, p->sigma_plane, 0};
}
RayzDenoiseGuidedParams denoise_params(const RayzDenoiseGuidedParams* p) {
    if (!p) return {0, RAYZ_DENOISE_DEFAULT_NORMAL_POWER_LOG2, RAYZ_DENOISE_ALBEDO, 0, RAYZ_DENOISE_GUIDED_DEFAULT_SIGMA_COLOR,
                    RAYZ_DENOISE_DEFAULT_SIGMA_PLANE, RAYZ_DENOISE_GUIDED_DEFAULT_VAR_FLOOR};
    return *p;
}

// A run of either mode; d_var_rgb and d_var_out belong to the guided one, and so does the tap: tap_level 0 is a run without one,
// otherwise d_tap receives the re-modulated colour after that many levels (rayz_hip_denoiser_run_guided_tap).
// Every argument is checked before the handle, and nothing here touches a device until all of them passed.
int denoiser_run(RayzDenoiser* dn, bool guided, const RayzDenoiseGuidedParams& p, const float* d_in, const float* d_var_rgb,
                 const RayzQueryOutputs* g, float* d_out, float* d_var_out, void* stream_arg, uint32_t tap_level = 0,
                 float* d_tap = nullptr) {
    if (p.levels > 8) return fail(RAYZ_ERR_BAD_ARG, "denoise levels %u > 8", p.levels);
    if (p.normal_power_log2 > 16) return fail(RAYZ_ERR_BAD_ARG, "denoise normal_power_log2 %u > 16", p.normal_power_log2);
    if (p.flags & ~kDenoiseFlags) return fail(RAYZ_ERR_BAD_ARG, "unknown denoise flag bits 0x%x", p.flags & ~kDenoiseFlags);
    const float sc = (float)p.sigma_color, sp = (float)p.sigma_plane, vf = (float)p.var_floor;
    const float sc2 = sc * sc, sp2 = sp * sp; // (what the kernels divide by: a sigma whose f32 square is 0 would divide 0 by 0)
    if (!(p.sigma_color > 0) || !(sc2 > 0)) return fail(RAYZ_ERR_BAD_ARG, "denoise sigma_color %g: must be positive (and its square in f32)", p.sigma_color);
    if (!(p.sigma_plane > 0) || !(sp2 > 0)) return fail(RAYZ_ERR_BAD_ARG, "denoise sigma_plane %g: must be positive (and its square in f32)", p.sigma_plane);
    // (den = sc2·(gv + vf) >= sc2·vf is what a guided tap divides by: were it 0, the centre tap would divide 0 by 0)
    if (guided && (!(p.var_floor > 0) || !(sc2 * vf > 0)))
        return fail(RAYZ_ERR_BAD_ARG, "denoise var_floor %g: must be positive (and sigma_color^2 x var_floor in f32)", p.var_floor);
    if (!d_in || !d_out) return fail(RAYZ_ERR_BAD_ARG, "denoise: null colour buffer");
    if (guided && !d_var_rgb) return fail(RAYZ_ERR_BAD_ARG, "denoise: the guided mode needs the per-channel variance (rayz_hip_progressive_noise_rgb)");
    RAYZ_TRY(frame_gbuffer_check("denoise", g));
    const bool demod = p.flags & RAYZ_DENOISE_ALBEDO;
    if (demod && !g->albedo) return fail(RAYZ_ERR_BAD_ARG, "denoise: RAYZ_DENOISE_ALBEDO needs the G-buffer's albedo");
    const uint32_t levels = p.levels ? p.levels : guided ? RAYZ_DENOISE_GUIDED_DEFAULT_LEVELS : RAYZ_DENOISE_DEFAULT_LEVELS;
    RAYZ_TRY(frame_handle_check(dn));
    hipStream_t st;
    RAYZ_TRY(frame_handle_stream(dn, stream_arg, st));
    DeviceScope scope(dn->device);
    RAYZ_TRY(frame_handle_wait_previous(dn, st)); // (a run of either mode)
    dn4 *const ga = dn->buf[0], *const gb = dn->buf[1], *const mod = dn->buf[2], *const col[2] = {dn->buf[3], dn->buf[4]};
    dn->levels_run = 0; // (a run that fails half-way leaves no timing)
    RAYZ_TRY(frame_handle_record(dn, 0, st));
    denoise_launch_pack(st, guided, d_in, d_var_rgb, g->index, (const float*)g->normal, (const float*)g->point,
                        demod ? (const float*)g->albedo : nullptr, dn->keys, ga, gb, mod, col[0], (size_t)dn->width * dn->height);
    RAYZ_TRY(frame_handle_launched(dn, 1, st));
    DenoiseArgs a{};
    a.ga = ga, a.gb = gb, a.mod = mod, a.rgb = d_out, a.var = d_var_out;
    a.width = dn->width, a.height = dn->height, a.normal_power_log2 = p.normal_power_log2, a.sp2 = sp2, a.sc2 = sc2, a.vf = vf;
    // which levels stage their taps in LDS: strides up to kDnLdsMaxStride (denoise.hpp) unless the measurement knob says otherwise
    const uint32_t lds_max = (uint32_t)tuning(RAYZ_DEBUG_DENOISE_LDS_STRIDE, kDnLdsMaxStride);
    for (uint32_t l = 0; l < levels; ++l) {
        a.src = col[l & 1], a.dst = col[(l & 1) ^ 1];
        a.stride = 1 << l, a.cl = (float)(1u << (2 * l));
        const bool lds = l <= (uint32_t)kDnMaxLdsLog2 && (1u << l) <= lds_max;
        a.tap = l + 1 == tap_level ? d_tap : nullptr;
        denoise_launch_level(st, guided, l + 1 == levels, a, l, lds);
        RAYZ_TRY(frame_handle_launched(dn, 2 + (int)l, st));
    }
    dn->levels_run = levels;
    return RAYZ_OK;
}

int denoiser_timing(RayzDenoiser* dn, uint32_t* levels, float* ms, uint32_t capacity) {
    RAYZ_TRY(frame_handle_check(dn));
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
    return guarded([&] { return frame_handle_create(device, width, height, out); });
}

int rayz_hip_denoiser_run(RayzDenoiser* dn, const RayzDenoiseParams* params, const float* d_rgb_in, const RayzQueryOutputs* gbuffer,
                          float* d_rgb_out, void* hip_stream) {
    return guarded([&] { return denoiser_run(dn, false, denoise_params(params), d_rgb_in, nullptr, gbuffer, d_rgb_out, nullptr, hip_stream); });
}

int rayz_hip_denoiser_run_guided(RayzDenoiser* dn, const RayzDenoiseGuidedParams* params, const float* d_rgb_in, const float* d_var_rgb,
                                 const RayzQueryOutputs* gbuffer, float* d_rgb_out, float* d_var_out_or_null, void* hip_stream) {
    return guarded([&] {
        return denoiser_run(dn, true, denoise_params(params), d_rgb_in, d_var_rgb, gbuffer, d_rgb_out, d_var_out_or_null, hip_stream);
    });
}

int rayz_hip_denoiser_run_guided_tap(RayzDenoiser* dn, const RayzDenoiseGuidedParams* params, const float* d_rgb_in, const float* d_var_rgb,
                                     const RayzQueryOutputs* gbuffer, float* d_rgb_out, float* d_var_out_or_null, uint32_t tap_level,
                                     float* d_tap_rgb, void* hip_stream) {
    return guarded([&] {
        const RayzDenoiseGuidedParams p = denoise_params(params);
        const uint32_t levels = p.levels ? p.levels : RAYZ_DENOISE_GUIDED_DEFAULT_LEVELS;
        if (!tap_level || tap_level > levels) return fail(RAYZ_ERR_BAD_ARG, "denoise tap_level %u: must lie in 1 .. levels = %u", tap_level, levels);
        if (!d_tap_rgb) return fail(RAYZ_ERR_BAD_ARG, "denoise: null tap buffer");
        if (d_tap_rgb == d_rgb_in || d_tap_rgb == d_rgb_out)
            return fail(RAYZ_ERR_BAD_ARG, "denoise: the tap buffer must be neither d_rgb_in nor d_rgb_out");
        return denoiser_run(dn, true, p, d_rgb_in, d_var_rgb, gbuffer, d_rgb_out, d_var_out_or_null, hip_stream, tap_level, d_tap_rgb);
    });
}

int rayz_hip_denoiser_set_keys(RayzDenoiser* dn, const uint32_t* d_keys_or_null) {
    return guarded([&] {
        RAYZ_TRY(frame_handle_check(dn));
        dn->keys = d_keys_or_null;
        return (int)RAYZ_OK;
    });
}

int rayz_hip_denoiser_timing(RayzDenoiser* dn, uint32_t* levels_or_null, float* ms_or_null, uint32_t capacity) {
    return guarded([&] { return denoiser_timing(dn, levels_or_null, ms_or_null, capacity); });
}

int rayz_hip_denoiser_destroy(RayzDenoiser* dn) {
    return guarded([&] { return frame_handle_free(dn); });
}

} // extern "C"
