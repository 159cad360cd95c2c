// upscaler.hpp — guided upscaling's handle (rayz_hip_upscaler_*; kernels and their launches: upscale.hpp; what it
// shares with the denoiser's and the temporal handle: frame_handle.hpp).
// Included by rayz_hip.hip; of the renderer it needs the device contexts only.
#pragma once

// The frame of the FrameHandle is the LOW-resolution one (its records are what the handle owns); full = factor x that.
// buf: ga, gb, mod, col, var of the low-resolution frame.  ev[0]: the run starts; ev[1]: packed; ev[2]: reconstructed.
// ev[3], ev[4]: around the footprint-albedo launch (§4.24), events of its own so that the last run's timing survives it.
struct RayzUpscaler : FrameHandle<5, 5> {
    static constexpr uint32_t kMagic = 0x55505a52u;
    static constexpr const char* kNoun = "upscaler";
    uint32_t factor = 0;
    uint32_t full_width = 0, full_height = 0;
    bool ran = false; // the last run was launched whole (false: none yet, or it failed half-way: no timing)
    bool footprint_ran = false; // the same for the last footprint-albedo call
};

namespace {

int upscale_factor_check(uint32_t factor) {
    if (factor < 2 || factor > 4) return fail(RAYZ_ERR_BAD_ARG, "upscale factor %u: must be 2, 3 or 4", factor);
    return RAYZ_OK;
}

struct UpscaleSpan { // a caller's buffer: where it starts and how many bytes a run touches
    const char* what;
    const void* p;
    size_t bytes;
};

// No output may overlap an input or another output.  (Before the handle is known every buffer counts as one pixel long: that finds
// equal pointers; with the handle's sizes it finds every overlap.)
int upscale_alias_check(const UpscaleSpan* in, int n_in, const UpscaleSpan* out, int n_out) {
    auto overlap = [](const UpscaleSpan& a, const UpscaleSpan& b) {
        if (!a.p || !b.p) return false;
        const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
        return a0 < b0 + b.bytes && b0 < a0 + a.bytes;
    };
    for (int o = 0; o < n_out; ++o) {
        for (int i = 0; i < n_in; ++i)
            if (overlap(out[o], in[i])) return fail(RAYZ_ERR_BAD_ARG, "upscale: output %s aliases input %s", out[o].what, in[i].what);
        for (int k = 0; k < o; ++k)
            if (overlap(out[o], out[k])) return fail(RAYZ_ERR_BAD_ARG, "upscale: output %s aliases output %s", out[o].what, out[k].what);
    }
    return RAYZ_OK;
}

int upscale_alias_check(const float* d_rgb_lo, const float* d_var_lo, const RayzQueryOutputs* lo, const RayzQueryOutputs* hi, bool demod,
                        float* d_out, float* d_var_out, uint8_t* d_stage, size_t n_lo, size_t n_hi) {
    const UpscaleSpan in[] = {{"d_rgb_lo", d_rgb_lo, n_lo * 12}, {"d_var_rgb_lo", d_var_lo, n_lo * 12},
                              {"gbuffer_lo.index", lo->index, n_lo * 4}, {"gbuffer_lo.normal", lo->normal, n_lo * 12},
                              {"gbuffer_lo.point", lo->point, n_lo * 12}, {"gbuffer_lo.albedo", demod ? lo->albedo : nullptr, n_lo * 12},
                              {"gbuffer_hi.index", hi->index, n_hi * 4}, {"gbuffer_hi.normal", hi->normal, n_hi * 12},
                              {"gbuffer_hi.point", hi->point, n_hi * 12}, {"gbuffer_hi.albedo", demod ? hi->albedo : nullptr, n_hi * 12}};
    const UpscaleSpan out[] = {{"d_rgb_out", d_out, n_hi * 12}, {"d_var_rgb_out", d_var_out, n_hi * 12}, {"d_stage_out", d_stage, n_hi}};
    return upscale_alias_check(in, (int)(sizeof(in) / sizeof(in[0])), out, 3);
}

// Every argument is checked before the handle, and nothing here touches a device until all of them passed.
// `phase` (rayz_hip_upscaler_run_phase): {phase_x, phase_y} of a lattice frame, or null for the run of block means.
int upscaler_run(RayzUpscaler* up, const RayzUpscaleParams* params, const uint32_t* phase, const float* d_rgb_lo, const float* d_var_lo,
                 const RayzQueryOutputs* lo, const RayzQueryOutputs* hi, float* d_out, float* d_var_out, uint8_t* d_stage, void* stream_arg) {
    if (!params) return fail(RAYZ_ERR_BAD_ARG, "upscale: null params (the factor has no default)");
    const RayzUpscaleParams& p = *params;
    RAYZ_TRY(upscale_factor_check(p.factor));
    if (phase && (phase[0] >= p.factor || phase[1] >= p.factor))
        return fail(RAYZ_ERR_BAD_ARG, "upscale phase (%u, %u): both below the factor %u", phase[0], phase[1], p.factor);
    if (p.normal_power_log2 > 16) return fail(RAYZ_ERR_BAD_ARG, "upscale normal_power_log2 %u > 16", p.normal_power_log2);
    if (p.flags & ~(uint32_t)RAYZ_DENOISE_ALBEDO) return fail(RAYZ_ERR_BAD_ARG, "unknown upscale flag bits 0x%x", p.flags & ~(uint32_t)RAYZ_DENOISE_ALBEDO);
    if (p.form > RAYZ_UPSCALE_FORM_DIRECT) return fail(RAYZ_ERR_BAD_ARG, "upscale form %u: this build has the direct form only (0 or 1)", p.form);
    const float sp = (float)p.sigma_plane, sp2 = sp * sp; // (what the kernel divides by, as the denoiser's)
    if (!(p.sigma_plane > 0) || !(sp2 > 0)) return fail(RAYZ_ERR_BAD_ARG, "upscale sigma_plane %g: must be positive (and its square in f32)", p.sigma_plane);
    if (!d_rgb_lo || !d_out) return fail(RAYZ_ERR_BAD_ARG, "upscale: null colour buffer");
    if (d_var_out && !d_var_lo) return fail(RAYZ_ERR_BAD_ARG, "upscale: a variance output needs the low-resolution variance");
    RAYZ_TRY(frame_gbuffer_check("upscale (low-resolution G-buffer)", lo));
    RAYZ_TRY(frame_gbuffer_check("upscale (full-size G-buffer)", hi));
    const bool demod = p.flags & RAYZ_DENOISE_ALBEDO;
    if (demod && (!lo->albedo || !hi->albedo)) return fail(RAYZ_ERR_BAD_ARG, "upscale: RAYZ_DENOISE_ALBEDO needs the albedo of both G-buffers");
    RAYZ_TRY(upscale_alias_check(d_rgb_lo, d_var_lo, lo, hi, demod, d_out, d_var_out, d_stage, 1, 1) /* equal pointers */);
    RAYZ_TRY(frame_handle_check(up));
    if (p.factor != up->factor) return fail(RAYZ_ERR_BAD_ARG, "upscale factor %u: the handle was created for %u", p.factor, up->factor);
    const size_t n_lo = (size_t)up->width * up->height, n_hi = (size_t)up->full_width * up->full_height;
    RAYZ_TRY(upscale_alias_check(d_rgb_lo, d_var_lo, lo, hi, demod, d_out, d_var_out, d_stage, n_lo, n_hi));
    hipStream_t st;
    RAYZ_TRY(frame_handle_stream(up, stream_arg, st));
    DeviceScope scope(up->device);
    RAYZ_TRY(frame_handle_wait_previous(up, st));
    dn4 *const ga = up->buf[0], *const gb = up->buf[1], *const mod = up->buf[2], *const col = up->buf[3], *const var = up->buf[4];
    up->ran = false;
    RAYZ_TRY(frame_handle_record(up, 0, st));
    denoise_launch_pack(st, false, d_rgb_lo, nullptr, lo->index, (const float*)lo->normal, (const float*)lo->point,
                        demod ? (const float*)lo->albedo : nullptr, nullptr, ga, gb, mod, col, n_lo);
    HIP_TRY(hipGetLastError());
    const bool with_var = d_var_lo && d_var_out; // (a variance nobody asked for is not packed)
    if (with_var) upscale_launch_pack_var(st, d_var_lo, mod, var, n_lo);
    RAYZ_TRY(frame_handle_launched(up, 1, st));
    UpscaleArgs a{};
    a.ga = ga, a.gb = gb, a.col = col, a.var = var, a.rgb_lo = d_rgb_lo;
    a.index = hi->index, a.normal = (const float*)hi->normal, a.point = (const float*)hi->point;
    a.albedo = demod ? (const float*)hi->albedo : nullptr;
    a.rgb = d_out, a.var_out = d_var_out, a.stage = d_stage;
    a.width = up->full_width, a.height = up->full_height, a.lo_width = up->width, a.lo_height = up->height, a.factor = up->factor;
    a.normal_power_log2 = p.normal_power_log2, a.sp2 = sp2;
    if (phase) {
        UpscalePhaseArgs pa{};
        pa.a = a, pa.var_lo = d_var_lo, pa.phase_x = phase[0], pa.phase_y = phase[1];
        upscale_launch_phase(st, with_var, pa);
    } else {
        upscale_launch(st, with_var, a);
    }
    RAYZ_TRY(frame_handle_launched(up, 2, st));
    up->ran = true;
    return RAYZ_OK;
}

int upscaler_timing(RayzUpscaler* up, float* pack_ms, float* upscale_ms) {
    RAYZ_TRY(frame_handle_check(up));
    if (!up->ran) return fail(RAYZ_ERR_STATE, "no upscaler run to time");
    DeviceScope scope(up->device);
    HIP_TRY(hipEventSynchronize(up->ev[2]));
    if (pack_ms) HIP_TRY(hipEventElapsedTime(pack_ms, up->ev[0], up->ev[1]));
    if (upscale_ms) HIP_TRY(hipEventElapsedTime(upscale_ms, up->ev[1], up->ev[2]));
    return RAYZ_OK;
}

// ---- the footprint albedo (§4.24; kernel and launch: footprint.hpp) -------------------------------------------------------------
int footprint_alias_check(const RayzQueryOutputs* lo, const RayzQueryOutputs* hi, float* d_out, uint8_t* d_count, size_t n_lo, size_t n_hi) {
    const UpscaleSpan in[] = {{"gbuffer_lo.index", lo->index, n_lo * 4}, {"gbuffer_lo.albedo", lo->albedo, n_lo * 12},
                              {"gbuffer_hi.index", hi->index, n_hi * 4}, {"gbuffer_hi.albedo", hi->albedo, n_hi * 12}};
    const UpscaleSpan out[] = {{"d_albedo_lo_out", d_out, n_lo * 12}, {"d_count_out", d_count, n_lo}};
    return upscale_alias_check(in, (int)(sizeof(in) / sizeof(in[0])), out, 2);
}

// Checked in upscaler_run's order: every argument before the handle, nothing touches a device until all of them passed.
int upscaler_footprint_albedo(RayzUpscaler* up, const RayzQueryOutputs* lo, const RayzQueryOutputs* hi, float* d_out, uint8_t* d_count,
                              void* stream_arg) {
    if (!lo || !hi) return fail(RAYZ_ERR_BAD_ARG, "footprint albedo: null G-buffer");
    if (!d_out) return fail(RAYZ_ERR_BAD_ARG, "footprint albedo: null output");
    if (!lo->index || !lo->albedo || !hi->index || !hi->albedo)
        return fail(RAYZ_ERR_BAD_ARG, "footprint albedo: both G-buffers need index and albedo");
    RAYZ_TRY(footprint_alias_check(lo, hi, d_out, d_count, 1, 1) /* equal pointers */);
    RAYZ_TRY(frame_handle_check(up));
    const size_t n_lo = (size_t)up->width * up->height, n_hi = (size_t)up->full_width * up->full_height;
    RAYZ_TRY(footprint_alias_check(lo, hi, d_out, d_count, n_lo, n_hi));
    hipStream_t st;
    RAYZ_TRY(frame_handle_stream(up, stream_arg, st));
    DeviceScope scope(up->device);
    RAYZ_TRY(frame_handle_wait_previous(up, st));
    up->footprint_ran = false;
    RAYZ_TRY(frame_handle_record(up, 3, st));
    rayz_dev_footprint::footprint_launch(st, up->factor, lo->index, (const float*)lo->albedo, hi->index, (const float*)hi->albedo, d_out,
                                         d_count, up->width, up->height);
    RAYZ_TRY(frame_handle_launched(up, 4, st));
    up->footprint_ran = true;
    return RAYZ_OK;
}

int upscaler_footprint_timing(RayzUpscaler* up, float* ms) {
    RAYZ_TRY(frame_handle_check(up));
    if (!up->footprint_ran) return fail(RAYZ_ERR_STATE, "no footprint-albedo call to time");
    DeviceScope scope(up->device);
    HIP_TRY(hipEventSynchronize(up->ev[4]));
    if (ms) HIP_TRY(hipEventElapsedTime(ms, up->ev[3], up->ev[4]));
    return RAYZ_OK;
}

} // namespace

extern "C" {

int rayz_hip_upscaler_create(int device, uint32_t width, uint32_t height, uint32_t factor, RayzUpscaler** out) {
    return guarded([&] {
        if (!out) return fail(RAYZ_ERR_BAD_ARG, "out handle pointer is null");
        *out = nullptr;
        RAYZ_TRY(upscale_factor_check(factor));
        if (!width || !height || width % factor || height % factor)
            return fail(RAYZ_ERR_BAD_ARG, "upscaler frame %ux%u: not a positive multiple of the factor %u in both directions", width, height, factor);
        if ((uint64_t)width * height > RAYZ_DENOISE_MAX_PIXELS)
            return fail(RAYZ_ERR_BAD_ARG, "upscaler frame %ux%u: more than RAYZ_DENOISE_MAX_PIXELS pixels", width, height);
        RAYZ_TRY(frame_handle_create(device, width / factor, height / factor, out));
        (*out)->factor = factor, (*out)->full_width = width, (*out)->full_height = height;
        return (int)RAYZ_OK;
    });
}

int rayz_hip_upscaler_run(RayzUpscaler* up, const RayzUpscaleParams* params, const float* d_rgb_lo, const float* d_var_rgb_lo_or_null,
                          const RayzQueryOutputs* gbuffer_lo, const RayzQueryOutputs* gbuffer_hi, float* d_rgb_out,
                          float* d_var_rgb_out_or_null, uint8_t* d_stage_out_or_null, void* hip_stream) {
    return guarded([&] {
        return upscaler_run(up, params, nullptr, d_rgb_lo, d_var_rgb_lo_or_null, gbuffer_lo, gbuffer_hi, d_rgb_out, d_var_rgb_out_or_null,
                            d_stage_out_or_null, hip_stream);
    });
}

int rayz_hip_upscaler_run_phase(RayzUpscaler* up, const RayzUpscaleParams* params, uint32_t phase_x, uint32_t phase_y, const float* d_rgb_lo,
                                const float* d_var_rgb_lo_or_null, const RayzQueryOutputs* gbuffer_lo, const RayzQueryOutputs* gbuffer_hi,
                                float* d_rgb_out, float* d_var_rgb_out_or_null, uint8_t* d_stage_out_or_null, void* hip_stream) {
    return guarded([&] {
        const uint32_t phase[2] = {phase_x, phase_y};
        return upscaler_run(up, params, phase, d_rgb_lo, d_var_rgb_lo_or_null, gbuffer_lo, gbuffer_hi, d_rgb_out, d_var_rgb_out_or_null,
                            d_stage_out_or_null, hip_stream);
    });
}

int rayz_hip_upscaler_timing(RayzUpscaler* up, float* pack_ms_or_null, float* upscale_ms_or_null) {
    return guarded([&] { return upscaler_timing(up, pack_ms_or_null, upscale_ms_or_null); });
}

int rayz_hip_upscaler_footprint_albedo(RayzUpscaler* up, const RayzQueryOutputs* gbuffer_lo, const RayzQueryOutputs* gbuffer_hi,
                                       float* d_albedo_lo_out, uint8_t* d_count_out_or_null, void* hip_stream) {
    return guarded([&] { return upscaler_footprint_albedo(up, gbuffer_lo, gbuffer_hi, d_albedo_lo_out, d_count_out_or_null, hip_stream); });
}

int rayz_hip_upscaler_footprint_timing(RayzUpscaler* up, float* ms) {
    return guarded([&] { return upscaler_footprint_timing(up, ms); });
}

int rayz_hip_upscaler_destroy(RayzUpscaler* up) {
    return guarded([&] { return frame_handle_free(up); });
}

} // extern "C"
