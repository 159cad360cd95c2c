// temporal_moments.hpp — the moments mode of temporal accumulation's handle (rayz_hip_temporal_track_moments, _step_moments;
// DESIGN.md §4.16; the kernel: temporal_moments_kernel.hpp; the handle and what both kinds of step share — temporal_run_step, the
// step's procedure —: temporal.hpp; the launch: temporal_kernel.hpp), its feedback mode (rayz_hip_temporal_track_feedback,
// _feedback; §4.17; temporal_feedback_kernel.hpp) and the choice of a moments step's kernel, temporal_launch_moments (the counts,
// background and clip kernels: temporal_modes_kernel.hpp; the cubic one: temporal_cubic_kernel.hpp).
// Included by rayz_hip.hip after temporal.hpp.
#pragma once

namespace {

// Only a handle without history may change its kind: a plain step's history has no moment records to go on from.
int temporal_track_moments(RayzTemporal* tm) {
    RAYZ_TRY(frame_handle_check(tm));
    if (tm->moments) return RAYZ_OK;
    if (tm->has_history)
        return fail(RAYZ_ERR_STATE, "temporal track_moments: the handle has history (call it after create or after rayz_hip_temporal_reset)");
    DeviceScope scope(tm->device);
    DevBuf<dn4> m[2];
    for (DevBuf<dn4>& b : m) {
        const hipError_t e = b.alloc((size_t)tm->width * tm->height);
        if (e != hipSuccess) return hip_fail(e, "temporal moment buffers"); // (m frees itself: the handle stays a plain one)
    }
    tm->mom[0] = std::move(m[0]), tm->mom[1] = std::move(m[1]);
    tm->moments = true;
    return RAYZ_OK;
}

// Only a moments handle without history may start to keep m1: a moments step's history has variances where m1 belongs.
// Allocates nothing: the v records change their meaning.
int temporal_track_feedback(RayzTemporal* tm) {
    RAYZ_TRY(frame_handle_check(tm));
    if (tm->feedback) return RAYZ_OK;
    if (!tm->moments) return fail(RAYZ_ERR_STATE, "temporal track_feedback: the handle is not in moments mode (rayz_hip_temporal_track_moments first)");
    if (tm->resampling == RAYZ_TEMPORAL_RESAMPLE_CUBIC)
        return fail(RAYZ_ERR_STATE, "temporal track_feedback: the handle is in cubic resampling mode (rayz_hip_temporal_set_resampling back to bilinear first)");
    if (tm->clip == RAYZ_TEMPORAL_CLIP_VARIANCE)
        return fail(RAYZ_ERR_STATE, "temporal track_feedback: the handle is in variance clip mode (rayz_hip_temporal_set_clip back to off first)");
    if (tm->background == RAYZ_TEMPORAL_BACKGROUND_ACCUMULATE)
        return fail(RAYZ_ERR_STATE, "temporal track_feedback: the handle accumulates the background (rayz_hip_temporal_set_background back to input first)");
    if (tm->has_history)
        return fail(RAYZ_ERR_STATE, "temporal track_feedback: the handle has history (call it after track_moments or after rayz_hip_temporal_reset)");
    tm->feedback = true;
    return RAYZ_OK;
}

// The colour of the side the last step wrote is replaced; the next step, a second feedback and _destroy wait for ev[2].
int temporal_feedback(RayzTemporal* tm, const float* d_rgb, void* stream_arg) {
    if (!d_rgb) return fail(RAYZ_ERR_BAD_ARG, "temporal feedback: null colour buffer");
    RAYZ_TRY(frame_handle_check(tm));
    if (!tm->feedback) return fail(RAYZ_ERR_STATE, "temporal feedback: the handle does not track feedback (rayz_hip_temporal_track_feedback first)");
    if (!tm->has_history) return fail(RAYZ_ERR_STATE, "temporal feedback: the handle has no history to write to (step it first)");
    hipStream_t st;
    RAYZ_TRY(frame_handle_stream(tm, stream_arg, st));
    DeviceScope scope(tm->device);
    RAYZ_TRY(frame_handle_wait_previous(tm, st)); // (the step that wrote this side, or an earlier feedback)
    temporal_feedback_launch_write(st, tm->buf[4 * tm->cur], d_rgb, tm->width, tm->height);
    RAYZ_TRY(frame_handle_launched(tm, 2, st));
    return RAYZ_OK;
}

// The launch of a moments step: the one place that says which kernel a moments handle's modes, the camera and the kind of step
// take.  (Behind the handle's check.  ACCUMULATE is never a feedback or a cubic handle: set_background refused them; a counts step
// is none either: temporal_run_step refused it; a cubic handle is no feedback handle: set_resampling refused it; and a static step
// of a cubic handle resamples nothing.)
void temporal_launch_moments(hipStream_t st, const RayzTemporal* tm, const RayzCameraDesc* cam, const TemporalMomentsArgs& a, bool is_static,
                             const uint32_t* d_counts) {
    const uint32_t w = a.t.width, h = a.t.height;
    const bool bg = tm->background == RAYZ_TEMPORAL_BACKGROUND_ACCUMULATE;
    if (temporal_clips(tm, is_static)) { // (§4.28: the moving step only; neither a counts, a cubic nor a feedback step)
        TemporalMomentsClipArgs c{{a, {}, nullptr}, temporal_clip_args(tm)};
        if (bg) temporal_background_args(tm, cam, is_static, c.m.G);
        hipLaunchKernelGGL(bg ? rayz_dev_clip::clip_moments_kernel<true> : rayz_dev_clip::clip_moments_kernel<false>, denoise_grid(w, h), dim3(256),
                           0, st, c);
    } else if (bg || d_counts) {
        TemporalMomentsModeArgs m{a, {}, d_counts};
        if (bg) temporal_background_args(tm, cam, is_static, m.G);
        void (*still)(TemporalMomentsModeArgs) = rayz_dev_counts::temporal_counts_moments_kernel<true>;
        void (*moving)(TemporalMomentsModeArgs) = rayz_dev_counts::temporal_counts_moments_kernel<false>;
        if (bg && d_counts)
            still = rayz_dev_bg::temporal_bg_counts_moments_kernel<true>, moving = rayz_dev_bg::temporal_bg_counts_moments_kernel<false>;
        else if (bg)
            still = rayz_dev_bg::temporal_bg_moments_kernel<true>, moving = rayz_dev_bg::temporal_bg_moments_kernel<false>;
        temporal_launch_step(st, still, moving, is_static, m, w, h);
    } else if (tm->resampling == RAYZ_TEMPORAL_RESAMPLE_CUBIC && !is_static)
        hipLaunchKernelGGL(rayz_dev_cubic::temporal_cubic_moments_step_kernel, denoise_grid(w, h), dim3(256), 0, st,
                           rayz_dev_cubic::TemporalCubicMomentsArgs{a, tm->taken});
    else if (tm->feedback)
        temporal_launch_step(st, temporal_feedback_step_kernel<true>, temporal_feedback_step_kernel<false>, is_static, a, w, h);
    else
        temporal_launch_step(st, temporal_moments_step_kernel<true>, temporal_moments_step_kernel<false>, is_static, a, w, h);
}

// Its own checks, then temporal.hpp's temporal_run_step: every argument is checked before the handle.
// d_counts: NULL for the step with one spp, else the counts step's array (§4.23), which stands for spp (then 0).
int temporal_step_moments(RayzTemporal* tm, const RayzTemporalParams* params, const RayzTemporalMomentsParams* mparams,
                          const RayzCameraDesc* cam, uint32_t spp, const uint32_t* d_counts, const float* d_in,
                          const RayzQueryOutputs* g, float* d_out, float* d_var_out, float* d_len_out, float* d_w2_out, void* stream_arg) {
    const RayzTemporalParams p = temporal_params_or_default(params);
    RayzTemporalMomentsParams mp{RAYZ_TEMPORAL_MOMENTS_DEFAULT_W2_MAX, RAYZ_TEMPORAL_MOMENTS_DEFAULT_MIN_TAPS};
    if (mparams) mp = *mparams;
    RAYZ_TRY(temporal_params_check(p, d_counts ? 1 : spp));
    if (!(mp.w2_max >= 0 && mp.w2_max <= 1)) return fail(RAYZ_ERR_BAD_ARG, "temporal w2_max %g: must lie in [0, 1]", mp.w2_max);
    if (!(mp.min_taps >= 2 && mp.min_taps <= 49)) return fail(RAYZ_ERR_BAD_ARG, "temporal min_taps %g: must lie in [2, 49]", mp.min_taps);
    if (!d_in || !d_out) return fail(RAYZ_ERR_BAD_ARG, "temporal: null colour buffer");
    if (!d_var_out) return fail(RAYZ_ERR_BAD_ARG, "temporal: null variance buffer");
    if (d_out == d_in)
        return fail(RAYZ_ERR_BAD_ARG, "temporal: a moments step cannot run in place (d_rgb_out == d_rgb_in: neighbours read the current frame)");
    const auto launch = [&](hipStream_t st, const TemporalArgs& t, bool is_static) { // (behind the handle's check: tm is a handle)
        TemporalMomentsArgs a{};
        a.t = t;
        a.prev_m = tm->mom[tm->cur], a.next_m = tm->mom[tm->cur ^ 1];
        a.w2_out = d_w2_out, a.wm = (float)mp.w2_max, a.mt = (float)mp.min_taps;
        temporal_launch_moments(st, tm, cam, a, is_static, d_counts);
    };
    return temporal_run_step(tm, true, p, cam, spp, d_in, nullptr, g, d_out, d_var_out, d_len_out, stream_arg, launch, d_counts != nullptr,
                             d_w2_out);
}

// The counts step of a moments handle (§4.23): its counts' checks, then the step above.
int temporal_step_moments_counts(RayzTemporal* tm, const RayzTemporalParams* params, const RayzTemporalMomentsParams* mparams,
                                 const RayzCameraDesc* cam, const uint32_t* d_counts, const float* d_in, const RayzQueryOutputs* g,
                                 float* d_out, float* d_var_out, float* d_len_out, float* d_w2_out, void* stream_arg) {
    RAYZ_TRY(temporal_counts_check(d_counts, {d_out, d_var_out, d_len_out, d_w2_out}));
    return temporal_step_moments(tm, params, mparams, cam, 0, d_counts, d_in, g, d_out, d_var_out, d_len_out, d_w2_out, stream_arg);
}

} // namespace

extern "C" {

int rayz_hip_temporal_track_moments(RayzTemporal* tm) {
    return guarded([&] { return temporal_track_moments(tm); });
}

int rayz_hip_temporal_track_feedback(RayzTemporal* tm) {
    return guarded([&] { return temporal_track_feedback(tm); });
}

int rayz_hip_temporal_feedback(RayzTemporal* tm, const float* d_rgb, void* hip_stream) {
    return guarded([&] { return temporal_feedback(tm, d_rgb, hip_stream); });
}

int rayz_hip_temporal_step_moments(RayzTemporal* tm, const RayzTemporalParams* params_or_null,
                                   const RayzTemporalMomentsParams* mparams_or_null, const RayzCameraDesc* camera, uint32_t spp,
                                   const float* d_rgb_in, const RayzQueryOutputs* gbuffer, float* d_rgb_out, float* d_var_out,
                                   float* d_length_out_or_null, float* d_w2_out_or_null, void* hip_stream) {
    return guarded([&] {
        return temporal_step_moments(tm, params_or_null, mparams_or_null, camera, spp, nullptr, d_rgb_in, gbuffer, d_rgb_out, d_var_out,
                                     d_length_out_or_null, d_w2_out_or_null, hip_stream);
    });
}

int rayz_hip_temporal_step_moments_counts(RayzTemporal* tm, const RayzTemporalParams* params_or_null,
                                          const RayzTemporalMomentsParams* mparams_or_null, const RayzCameraDesc* camera,
                                          const uint32_t* d_counts, const float* d_rgb_in, const RayzQueryOutputs* gbuffer,
                                          float* d_rgb_out, float* d_var_out, float* d_length_out_or_null, float* d_w2_out_or_null,
                                          void* hip_stream) {
    return guarded([&] {
        return temporal_step_moments_counts(tm, params_or_null, mparams_or_null, camera, d_counts, d_rgb_in, gbuffer, d_rgb_out,
                                            d_var_out, d_length_out_or_null, d_w2_out_or_null, hip_stream);
    });
}

} // extern "C"
