// temporal.hpp — temporal accumulation's handle (rayz_hip_temporal_*; the kernel and its launch:
// temporal_kernel.hpp; what it shares with the denoiser's handle: frame_handle.hpp; the moments mode: temporal_moments.hpp) and
// the one procedure of a step of either kind, temporal_run_step; the background mode's host part and calls (§4.27); the choice of a
// plain step's kernel, temporal_launch_plain (the counts, background, cubic and clip kernels: temporal_modes_kernel.hpp); the clip
// mode's calls (§4.28).
// Included by rayz_hip.hip; of the renderer it needs the device contexts only.
#pragma once

// buf: ping-pong x {colour + length, variance, normal + index, point}.  ev[0]: the step starts; ev[1]: it is done; ev[2]: the
// feedback written behind it is done (rayz_hip_temporal_feedback; an event of its own, so that ev[0] .. ev[1] stays the step's time).
struct RayzTemporal : FrameHandle<2 * 4, 3> {
    static constexpr uint32_t kMagic = 0x544d5a52u;
    static constexpr const char* kNoun = "temporal";
    int cur = 0;            // the side of buf the last step wrote: what the next step reads
    bool has_history = false;
    RayzCameraDesc cam{};   // the last step's camera, with its M and from: what the next step projects with
    float M[9] = {}, from[3] = {};
    bool timed = false;     // the last step ran to its end: ev[0] .. ev[1] is its time
    bool moments = false;   // rayz_hip_temporal_track_moments: the handle takes _step_moments and not _step (§4.16)
    DevBuf<dn4> mom[2];     // .. and owns, per ping-pong side, one more record per pixel {m2.r, m2.g, m2.b, W2}; empty otherwise
    bool feedback = false;  // rayz_hip_temporal_track_feedback: a moments handle whose variance records hold the raw first moment
                            // m1 instead, and which takes rayz_hip_temporal_feedback (§4.17)
    uint32_t resampling = RAYZ_TEMPORAL_RESAMPLE_BILINEAR; // rayz_hip_temporal_set_resampling (§4.26): how a moving step fetches the colour history
    uint8_t* taken = nullptr; // .. and the caller's device bytes every step writes (1: the pixel took the cubic path), or NULL
    uint32_t background = RAYZ_TEMPORAL_BACKGROUND_INPUT; // rayz_hip_temporal_set_background (§4.27): whether a pixel with id < 0 gathers history
    uint32_t clip = RAYZ_TEMPORAL_CLIP_OFF; // rayz_hip_temporal_set_clip (§4.28): whether a moving step clamps the colour history ..
    RayzTemporalClipParams clip_params{RAYZ_TEMPORAL_CLIP_DEFAULT_GAMMA, RAYZ_TEMPORAL_CLIP_DEFAULT_MIN_TAPS}; // .. to what box ..
    uint8_t* clipped = nullptr; // .. and the caller's device bytes every step writes (1: a channel was clipped), or NULL
};

namespace {

// What §4.15's and §4.27's host parts share of a camera with u = px_du, v = px_dv, a = px_origin − look_from, f64, every operation
// written out: the rows r0 = v×a, r1 = a×u, r2 = u×v; returns det = u·r0.
double temporal_camera_rows(const RayzCameraDesc* c, double (&r)[3][3]) {
    const double *u = c->px_du, *v = c->px_dv;
    const double a[3] = {c->px_origin[0] - c->look_from[0], c->px_origin[1] - c->look_from[1], c->px_origin[2] - c->look_from[2]};
    auto cross = [](const double* p, const double* q, double* o) {
        o[0] = p[1] * q[2] - p[2] * q[1];
        o[1] = p[2] * q[0] - p[0] * q[2];
        o[2] = p[0] * q[1] - p[1] * q[0];
    };
    cross(v, a, r[0]);
    cross(a, u, r[1]);
    cross(u, v, r[2]);
    return (u[0] * r[0][0] + u[1] * r[0][1]) + u[2] * r[0][2];
}

// The host part of a step (§4.15): M = the inverse of the matrix with columns px_du, px_dv and px_origin − look_from, each entry
// rounded once to f32, and look_from in f32.  False: det is zero or not finite.
bool temporal_camera_matrix(const RayzCameraDesc* c, float* M, float* from) {
    double r[3][3];
    const double det = temporal_camera_rows(c, r);
    if (!(det != 0.0) || !std::isfinite(det)) return false;
    for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 3; ++j) M[3 * k + j] = (float)(r[k][j] / det);
    for (int j = 0; j < 3; ++j) from[j] = (float)c->look_from[j];
    return true;
}

// The host part of a step in ACCUMULATE mode (§4.27), f64: G = the previous camera's rows over its det, times the matrix with
// columns px_du, px_dv and px_origin − look_from of this step's camera, each entry rounded once to f32 — this frame's pixel centre
// (x, y, 1) to s·(x', y', 1) in the previous frame.  prev was a step's camera: its det passed temporal_camera_matrix.
void temporal_background_matrix(const RayzCameraDesc* prev, const RayzCameraDesc* cam, float* G) {
    double r[3][3];
    const double det = temporal_camera_rows(prev, r);
    const double a[3] = {cam->px_origin[0] - cam->look_from[0], cam->px_origin[1] - cam->look_from[1], cam->px_origin[2] - cam->look_from[2]};
    const double* c[3] = {cam->px_du, cam->px_dv, a};
    for (int k = 0; k < 3; ++k)
        for (int j = 0; j < 3; ++j) G[3 * k + j] = (float)(((r[k][0] * c[j][0] + r[k][1] * c[j][1]) + r[k][2] * c[j][2]) / det);
}

// G as the background kernels take it: zeros where no pixel reads it (no history, or a static step).
void temporal_background_args(const RayzTemporal* tm, const RayzCameraDesc* cam, bool is_static, float* G) {
    std::memset(G, 0, 9 * sizeof(float));
    if (tm->has_history && !is_static) temporal_background_matrix(&tm->cam, cam, G);
}

// §4.28: does this step of the handle run a clip kernel?  Only a moving step with history of a VARIANCE handle does (which is no
// counts step, and whose handle neither tracks feedback nor resamples cubically: all refused before).
bool temporal_clips(const RayzTemporal* tm, bool is_static) {
    return tm->clip == RAYZ_TEMPORAL_CLIP_VARIANCE && tm->has_history && !is_static;
}

// .. and what its kernel takes of the handle.
TemporalClip temporal_clip_args(const RayzTemporal* tm) {
    return TemporalClip{(float)tm->clip_params.gamma, (float)tm->clip_params.min_taps, tm->clipped};
}

// The checks both kinds of step make of the parameters and the sample count ..
int temporal_params_check(const RayzTemporalParams& p, uint32_t spp) {
    if (!(p.alpha_min >= 0 && p.alpha_min <= 1)) return fail(RAYZ_ERR_BAD_ARG, "temporal alpha_min %g: must lie in [0, 1]", p.alpha_min);
    if (!(p.n_max >= 1)) return fail(RAYZ_ERR_BAD_ARG, "temporal n_max %g: must be at least 1", p.n_max);
    if (!(p.normal_cos_min >= -1 && p.normal_cos_min <= 1))
        return fail(RAYZ_ERR_BAD_ARG, "temporal normal_cos_min %g: must lie in [-1, 1]", p.normal_cos_min);
    if (!(p.max_rel_dist > 0)) return fail(RAYZ_ERR_BAD_ARG, "temporal max_rel_dist %g: must be positive", p.max_rel_dist);
    if (!spp || spp > (1u << 24)) return fail(RAYZ_ERR_BAD_ARG, "temporal spp %u: must lie in 1 .. 2^24 (it is used as f32)", spp);
    return RAYZ_OK;
}

// .. and of the guides and the camera, whose M and from they return.
int temporal_frame_check(const RayzQueryOutputs* g, const RayzCameraDesc* cam, float* M, float* from) {
    RAYZ_TRY(frame_gbuffer_check("temporal", g));
    if (!cam) return fail(RAYZ_ERR_BAD_ARG, "temporal: null camera");
    if (!temporal_camera_matrix(cam, M, from))
        return fail(RAYZ_ERR_BAD_ARG, "temporal: the camera's px_du, px_dv and px_origin - look_from span no volume (det is 0 or not finite)");
    return RAYZ_OK;
}

// The kernel's arguments of a step of either kind (d_var: the plain step's variance input, or NULL).
TemporalArgs temporal_args(const RayzTemporal* tm, const RayzTemporalParams& p, uint32_t spp, const float* d_in, const float* d_var,
                           const RayzQueryOutputs* g, float* d_out, float* d_var_out, float* d_len_out) {
    const float r = (float)p.max_rel_dist;
    TemporalArgs a{};
    a.rgb = d_in, a.var = d_var, a.index = g->index, a.normal = (const float*)g->normal, a.point = (const float*)g->point;
    const DevBuf<dn4>*prev = tm->buf + 4 * tm->cur, *next = tm->buf + 4 * (tm->cur ^ 1);
    a.prev = TemporalHistory{prev[0], prev[1], prev[2], prev[3]};
    a.next = TemporalHistory{next[0], next[1], next[2], next[3]};
    a.rgb_out = d_out, a.var_out = d_var_out, a.len_out = d_len_out;
    a.width = tm->width, a.height = tm->height, a.has_history = tm->has_history;
    std::memcpy(a.M, tm->M, sizeof(a.M));
    std::memcpy(a.from, tm->from, sizeof(a.from));
    a.spp = (float)spp, a.am = (float)p.alpha_min, a.nm = (float)p.n_max, a.cm = (float)p.normal_cos_min, a.r2 = r * r;
    return a;
}

// The step is enqueued: the handle now describes the history it leaves.
void temporal_stepped(RayzTemporal* tm, const RayzCameraDesc* cam, const float* M, const float* from) {
    tm->cur ^= 1, tm->has_history = true, tm->cam = *cam, tm->timed = true;
    std::memcpy(tm->M, M, sizeof(tm->M));
    std::memcpy(tm->from, from, sizeof(tm->from));
}

// The parameters a step takes where the caller gives none.
RayzTemporalParams temporal_params_or_default(const RayzTemporalParams* params) {
    return params ? *params
                  : RayzTemporalParams{RAYZ_TEMPORAL_DEFAULT_ALPHA_MIN, RAYZ_TEMPORAL_DEFAULT_N_MAX, RAYZ_TEMPORAL_DEFAULT_NORMAL_COS_MIN,
                                       RAYZ_TEMPORAL_DEFAULT_MAX_REL_DIST};
}

// What a step of either kind does once its own parameters and buffers are checked: the last checks — of the guides and the
// camera, of the handle and of its mode (moments: the kind of handle this step takes) — and then the step on the handle's stream
// behind the previous one.  launch(stream, the plain step's arguments, is_static) completes the mode's arguments and launches.
// Every argument is checked before the handle, and nothing here touches a device until all of them passed.
// counts: this is a counts step (§4.23: spp is 0 and the launch brings a count per pixel), which neither a feedback handle nor one in
// cubic mode (§4.26) takes.  d_w2_out: the moments step's fourth output, which like the other three the handle's taken bytes must not be.
template <class Launch>
int temporal_run_step(RayzTemporal* tm, bool moments, const RayzTemporalParams& p, const RayzCameraDesc* cam, uint32_t spp,
                      const float* d_in, const float* d_var, const RayzQueryOutputs* g, float* d_out, float* d_var_out, float* d_len_out,
                      void* stream_arg, const Launch& launch, bool counts = false, const float* d_w2_out = nullptr) {
    float M[9], from[3];
    RAYZ_TRY(temporal_frame_check(g, cam, M, from));
    RAYZ_TRY(frame_handle_check(tm));
    if (tm->moments != moments)
        return fail(RAYZ_ERR_STATE, "%s",
                    moments ? "a plain temporal handle takes rayz_hip_temporal_step (rayz_hip_temporal_track_moments first)"
                            : "a temporal handle in moments mode takes rayz_hip_temporal_step_moments");
    if (counts && tm->feedback)
        return fail(RAYZ_ERR_STATE, "a temporal handle that tracks feedback takes no counts step (its first moment has no rule for a pixel without samples)");
    if (counts && tm->resampling == RAYZ_TEMPORAL_RESAMPLE_CUBIC)
        return fail(RAYZ_ERR_STATE, "a temporal handle in cubic resampling mode takes no counts step (rayz_hip_temporal_set_resampling back to bilinear first)");
    if (counts && tm->clip == RAYZ_TEMPORAL_CLIP_VARIANCE)
        return fail(RAYZ_ERR_STATE, "a temporal handle in variance clip mode takes no counts step (rayz_hip_temporal_set_clip back to off first)");
    if (tm->taken)
        for (const void* o : {(const void*)d_out, (const void*)d_var_out, (const void*)d_len_out, (const void*)d_w2_out})
            if (o == (const void*)tm->taken) return fail(RAYZ_ERR_BAD_ARG, "temporal: the handle's d_taken is also an output of the step");
    if (tm->clipped)
        for (const void* o : {(const void*)d_out, (const void*)d_var_out, (const void*)d_len_out, (const void*)d_w2_out, (const void*)tm->taken})
            if (o == (const void*)tm->clipped)
                return fail(RAYZ_ERR_BAD_ARG, "temporal: the handle's d_clipped is also an output of the step or its d_taken");
    hipStream_t st;
    RAYZ_TRY(frame_handle_stream(tm, stream_arg, st));
    DeviceScope scope(tm->device);
    RAYZ_TRY(frame_handle_wait_previous(tm, st)); // (this step reads what the previous one wrote)
    const bool is_static = tm->has_history && std::memcmp(cam, &tm->cam, sizeof(RayzCameraDesc)) == 0;
    const TemporalArgs a = temporal_args(tm, p, spp, d_in, d_var, g, d_out, d_var_out, d_len_out);
    tm->timed = false; // (a step that fails half-way leaves no timing)
    RAYZ_TRY(frame_handle_record(tm, 0, st));
    // (§4.26: only the cubic kernels write the taken bytes themselves; every other step took the sixteen taps nowhere)
    const bool cubic = tm->resampling == RAYZ_TEMPORAL_RESAMPLE_CUBIC && !is_static;
    if (tm->taken && !cubic) HIP_TRY(hipMemsetAsync(tm->taken, 0, (size_t)tm->width * tm->height, st));
    // (§4.28: only the clip kernels write the clipped bytes themselves; every other step clipped nothing)
    if (tm->clipped && !temporal_clips(tm, is_static)) HIP_TRY(hipMemsetAsync(tm->clipped, 0, (size_t)tm->width * tm->height, st));
    launch(st, a, is_static);
    RAYZ_TRY(frame_handle_launched(tm, 1, st));
    temporal_stepped(tm, cam, M, from);
    return RAYZ_OK;
}

// What both counts steps (§4.23) check of their counts: every pixel reads its own and, in the moments step, its neighbours', so
// the array is no output of the step.
int temporal_counts_check(const uint32_t* d_counts, std::initializer_list<const void*> outputs) {
    if (!d_counts) return fail(RAYZ_ERR_BAD_ARG, "temporal: null counts buffer");
    for (const void* o : outputs)
        if (o == (const void*)d_counts) return fail(RAYZ_ERR_BAD_ARG, "temporal: d_counts is also an output of the step");
    return RAYZ_OK;
}

// The launch of a plain step: the one place that says which kernel a plain handle's modes, the camera and the kind of step take.
// (Behind the handle's check.  ACCUMULATE is never a cubic handle: set_background refused it; a counts step is none either:
// temporal_run_step refused it; and a static step of a cubic handle resamples nothing.)
void temporal_launch_plain(hipStream_t st, const RayzTemporal* tm, const RayzCameraDesc* cam, const TemporalArgs& a, bool is_static,
                           const uint32_t* d_counts) {
    const bool bg = tm->background == RAYZ_TEMPORAL_BACKGROUND_ACCUMULATE;
    const bool cubic = tm->resampling == RAYZ_TEMPORAL_RESAMPLE_CUBIC && !is_static;
    if (temporal_clips(tm, is_static)) { // (§4.28: the moving step only; neither a counts nor a cubic step)
        TemporalClipArgs c{{a, {}, nullptr, nullptr}, temporal_clip_args(tm)};
        if (bg) temporal_background_args(tm, cam, is_static, c.m.G);
        hipLaunchKernelGGL(bg ? rayz_dev_clip::clip_plain_kernel<true> : rayz_dev_clip::clip_plain_kernel<false>, denoise_grid(a.width, a.height),
                           dim3(256), 0, st, c);
        return;
    }
    if (!bg && !d_counts && !cubic)
        return temporal_launch_step(st, temporal_step_kernel<true>, temporal_step_kernel<false>, is_static, a, a.width, a.height);
    TemporalModeArgs m{a, {}, d_counts, tm->taken};
    if (bg) temporal_background_args(tm, cam, is_static, m.G);
    void (*still)(TemporalModeArgs) = nullptr; // (the cubic step has no static form)
    void (*moving)(TemporalModeArgs) = rayz_dev_cubic::temporal_cubic_step_kernel;
    if (bg && d_counts)
        still = rayz_dev_bg::temporal_bg_counts_kernel<true>, moving = rayz_dev_bg::temporal_bg_counts_kernel<false>;
    else if (bg)
        still = rayz_dev_bg::temporal_bg_kernel<true>, moving = rayz_dev_bg::temporal_bg_kernel<false>;
    else if (d_counts)
        still = rayz_dev_counts::temporal_counts_kernel<true>, moving = rayz_dev_counts::temporal_counts_kernel<false>;
    temporal_launch_step(st, still, moving, is_static, m, a.width, a.height);
}

// The step of a plain handle.  counts: the counts step (§4.23), a count per pixel for spp (then 0; the kernel does not read the
// arguments' spp) — d_counts is checked behind the buffers; else d_counts is NULL.
int temporal_step(RayzTemporal* tm, const RayzTemporalParams* params, const RayzCameraDesc* cam, uint32_t spp, bool counts,
                  const uint32_t* d_counts, const float* d_in, const float* d_var, const RayzQueryOutputs* g, float* d_out,
                  float* d_var_out, float* d_len_out, void* stream_arg) {
    const RayzTemporalParams p = temporal_params_or_default(params);
    RAYZ_TRY(temporal_params_check(p, counts ? 1 : spp));
    if (!d_in || !d_out) return fail(RAYZ_ERR_BAD_ARG, "temporal: null colour buffer");
    if (!d_var || !d_var_out) return fail(RAYZ_ERR_BAD_ARG, "temporal: null variance buffer (rayz_hip_progressive_noise_rgb writes the input)");
    if (counts) RAYZ_TRY(temporal_counts_check(d_counts, {d_out, d_var_out, d_len_out}));
    const auto launch = [&](hipStream_t st, const TemporalArgs& a, bool is_static) { temporal_launch_plain(st, tm, cam, a, is_static, d_counts); };
    return temporal_run_step(tm, false, p, cam, spp, d_in, d_var, g, d_out, d_var_out, d_len_out, stream_arg, launch, counts);
}

// §4.26's mode and the taken bytes.  The mode is an argument and is checked before the handle, as a step's arguments are.
int temporal_set_resampling(RayzTemporal* tm, uint32_t mode, uint8_t* d_taken) {
    if (mode != RAYZ_TEMPORAL_RESAMPLE_BILINEAR && mode != RAYZ_TEMPORAL_RESAMPLE_CUBIC)
        return fail(RAYZ_ERR_BAD_ARG, "temporal resampling mode %u: must be RAYZ_TEMPORAL_RESAMPLE_BILINEAR or _CUBIC", mode);
    RAYZ_TRY(frame_handle_check(tm));
    if (mode == RAYZ_TEMPORAL_RESAMPLE_CUBIC && tm->feedback)
        return fail(RAYZ_ERR_STATE, "temporal set_resampling: a handle that tracks feedback has no cubic mode (its raw first moment has no resampling rule)");
    if (mode == RAYZ_TEMPORAL_RESAMPLE_CUBIC && tm->background == RAYZ_TEMPORAL_BACKGROUND_ACCUMULATE)
        return fail(RAYZ_ERR_STATE, "temporal set_resampling: a handle that accumulates the background has no cubic mode (rayz_hip_temporal_set_background back to input first)");
    if (mode == RAYZ_TEMPORAL_RESAMPLE_CUBIC && tm->clip == RAYZ_TEMPORAL_CLIP_VARIANCE)
        return fail(RAYZ_ERR_STATE, "temporal set_resampling: a handle in variance clip mode has no cubic mode (rayz_hip_temporal_set_clip back to off first)");
    tm->resampling = mode, tm->taken = d_taken;
    return RAYZ_OK;
}

int temporal_get_resampling(RayzTemporal* tm, uint32_t* mode) {
    RAYZ_TRY(frame_handle_check(tm));
    if (mode) *mode = tm->resampling;
    return RAYZ_OK;
}

// §4.27's mode.  The mode is an argument and is checked before the handle, as a step's arguments are.
int temporal_set_background(RayzTemporal* tm, uint32_t mode) {
    if (mode != RAYZ_TEMPORAL_BACKGROUND_INPUT && mode != RAYZ_TEMPORAL_BACKGROUND_ACCUMULATE)
        return fail(RAYZ_ERR_BAD_ARG, "temporal background mode %u: must be RAYZ_TEMPORAL_BACKGROUND_INPUT or _ACCUMULATE", mode);
    RAYZ_TRY(frame_handle_check(tm));
    if (mode == RAYZ_TEMPORAL_BACKGROUND_ACCUMULATE && tm->feedback)
        return fail(RAYZ_ERR_STATE, "temporal set_background: a handle that tracks feedback does not accumulate the background (its steps have no background kernels)");
    if (mode == RAYZ_TEMPORAL_BACKGROUND_ACCUMULATE && tm->resampling == RAYZ_TEMPORAL_RESAMPLE_CUBIC)
        return fail(RAYZ_ERR_STATE, "temporal set_background: a handle in cubic resampling mode does not accumulate the background (rayz_hip_temporal_set_resampling back to bilinear first)");
    tm->background = mode;
    return RAYZ_OK;
}

int temporal_get_background(RayzTemporal* tm, uint32_t* mode) {
    RAYZ_TRY(frame_handle_check(tm));
    if (mode) *mode = tm->background;
    return RAYZ_OK;
}

// §4.28's mode, its parameters and the clipped bytes.  The mode and the parameters are arguments and are checked before the handle.
int temporal_set_clip(RayzTemporal* tm, uint32_t mode, const RayzTemporalClipParams* params, uint8_t* d_clipped) {
    if (mode != RAYZ_TEMPORAL_CLIP_OFF && mode != RAYZ_TEMPORAL_CLIP_VARIANCE)
        return fail(RAYZ_ERR_BAD_ARG, "temporal clip mode %u: must be RAYZ_TEMPORAL_CLIP_OFF or _VARIANCE", mode);
    const RayzTemporalClipParams p = params ? *params : RayzTemporalClipParams{RAYZ_TEMPORAL_CLIP_DEFAULT_GAMMA, RAYZ_TEMPORAL_CLIP_DEFAULT_MIN_TAPS};
    if (!(p.gamma >= 0)) return fail(RAYZ_ERR_BAD_ARG, "temporal clip gamma %g: must be at least 0 (+inf never clips)", p.gamma);
    if (!(p.min_taps >= 2 && p.min_taps <= 49)) return fail(RAYZ_ERR_BAD_ARG, "temporal clip min_taps %g: must lie in [2, 49]", p.min_taps);
    RAYZ_TRY(frame_handle_check(tm));
    if (mode == RAYZ_TEMPORAL_CLIP_VARIANCE && tm->feedback)
        return fail(RAYZ_ERR_STATE, "temporal set_clip: a handle that tracks feedback has no clip mode (its raw first moment has no clip rule)");
    if (mode == RAYZ_TEMPORAL_CLIP_VARIANCE && tm->resampling == RAYZ_TEMPORAL_RESAMPLE_CUBIC)
        return fail(RAYZ_ERR_STATE, "temporal set_clip: a handle in cubic resampling mode has no clip mode (rayz_hip_temporal_set_resampling back to bilinear first)");
    tm->clip = mode, tm->clip_params = p, tm->clipped = d_clipped;
    return RAYZ_OK;
}

int temporal_get_clip(RayzTemporal* tm, uint32_t* mode, RayzTemporalClipParams* params) {
    RAYZ_TRY(frame_handle_check(tm));
    if (mode) *mode = tm->clip;
    if (params) *params = tm->clip_params;
    return RAYZ_OK;
}

int temporal_reset(RayzTemporal* tm) {
    RAYZ_TRY(frame_handle_check(tm));
    tm->has_history = false; // (the buffers keep their bytes; no step reads them before it has written them)
    return RAYZ_OK;
}

int temporal_timing(RayzTemporal* tm, float* ms) {
    RAYZ_TRY(frame_handle_check(tm));
    if (!tm->timed) return fail(RAYZ_ERR_STATE, "no temporal step to time");
    DeviceScope scope(tm->device);
    HIP_TRY(hipEventSynchronize(tm->ev[1]));
    if (ms) HIP_TRY(hipEventElapsedTime(ms, tm->ev[0], tm->ev[1]));
    return RAYZ_OK;
}

} // namespace

extern "C" {

int rayz_hip_temporal_create(int device, uint32_t width, uint32_t height, RayzTemporal** out) {
    return guarded([&] { return frame_handle_create(device, width, height, out); });
}

int rayz_hip_temporal_step(RayzTemporal* tm, const RayzTemporalParams* params_or_null, const RayzCameraDesc* camera, uint32_t spp,
                           const float* d_rgb_in, const float* d_var_rgb, const RayzQueryOutputs* gbuffer, float* d_rgb_out,
                           float* d_var_out, float* d_length_out_or_null, void* hip_stream) {
    return guarded([&] {
        return temporal_step(tm, params_or_null, camera, spp, false, nullptr, d_rgb_in, d_var_rgb, gbuffer, d_rgb_out, d_var_out,
                             d_length_out_or_null, hip_stream);
    });
}

int rayz_hip_temporal_step_counts(RayzTemporal* tm, const RayzTemporalParams* params_or_null, const RayzCameraDesc* camera,
                                  const uint32_t* d_counts, const float* d_rgb_in, const float* d_var_rgb, const RayzQueryOutputs* gbuffer,
                                  float* d_rgb_out, float* d_var_out, float* d_length_out_or_null, void* hip_stream) {
    return guarded([&] {
        return temporal_step(tm, params_or_null, camera, 0, true, d_counts, d_rgb_in, d_var_rgb, gbuffer, d_rgb_out, d_var_out,
                             d_length_out_or_null, hip_stream);
    });
}

int rayz_hip_temporal_set_resampling(RayzTemporal* tm, uint32_t mode, uint8_t* d_taken_or_null) {
    return guarded([&] { return temporal_set_resampling(tm, mode, d_taken_or_null); });
}

int rayz_hip_temporal_get_resampling(RayzTemporal* tm, uint32_t* mode) {
    return guarded([&] { return temporal_get_resampling(tm, mode); });
}

int rayz_hip_temporal_set_background(RayzTemporal* tm, uint32_t mode) {
    return guarded([&] { return temporal_set_background(tm, mode); });
}

int rayz_hip_temporal_get_background(RayzTemporal* tm, uint32_t* mode) {
    return guarded([&] { return temporal_get_background(tm, mode); });
}

int rayz_hip_temporal_set_clip(RayzTemporal* tm, uint32_t mode, const RayzTemporalClipParams* params_or_null, uint8_t* d_clipped_or_null) {
    return guarded([&] { return temporal_set_clip(tm, mode, params_or_null, d_clipped_or_null); });
}

int rayz_hip_temporal_get_clip(RayzTemporal* tm, uint32_t* mode, RayzTemporalClipParams* params_or_null) {
    return guarded([&] { return temporal_get_clip(tm, mode, params_or_null); });
}

int rayz_hip_temporal_reset(RayzTemporal* tm) {
    return guarded([&] { return temporal_reset(tm); });
}

int rayz_hip_temporal_timing(RayzTemporal* tm, float* ms) {
    return guarded([&] { return temporal_timing(tm, ms); });
}

int rayz_hip_temporal_destroy(RayzTemporal* tm) {
    return guarded([&] { return frame_handle_free(tm); });
}

} // extern "C"
