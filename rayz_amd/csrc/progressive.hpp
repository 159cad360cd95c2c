// progressive.hpp — progressive rendering (rayz_hip_progressive_*): the frame in passes of whole chunks, and the noise estimate of
// a tracked handle.  Included by rayz_hip.hip, behind the trace launch it drives (prepare_scene, trace_window).
#pragma once

// A pass traces a window of chunks [c0, c1) into the scene's workspace and folds the window's chunk sums into the handle's
// accumulator in chunk order (accumulate_kernel).  The chunk sums do not depend on the window (trace_window), and the fold
// performs resolve_kernel's additions in resolve_kernel's order, so once every chunk is covered the frame is the one-shot
// render's, bit for bit, whatever the passes were.
struct RayzProgressive {
    RayzScene* scene = nullptr;
    int device = -1;
    RayzCameraDesc cam{};
    RayzRenderParams params{};
    std::vector<uint32_t> starts;           // the chunk schedule: n_chunks + 1 entries
    DevBuf<uint32_t> d_starts;              // the handle's own device copy (the scene's table follows the scene's last render)
    DevBytes acc;                           // shard_pixels running sums (r4 of the precision)
    DevBuf<unsigned long long> counters;    // [0] queue head (cleared per pass), [1..3] summed over the passes
    PrimaryLists primary;                   // the shard's primary lists: built by the first pass that uses them — the camera and params are the handle's
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
    // adaptive mode (rayz_hip_progressive_set_adaptive; adaptive_passes.hpp): absent from any other handle
    bool adaptive = false;
    uint32_t min_chunks = 0;
    DevBuf<uint32_t> frozen_at;             // shard_pixels: 0 = active, else the chunk count the pixel froze at
    DevBuf<uint32_t> active[2];             // the active list of the next pass (active[cur]) and the one being built
    DevBuf<uint32_t> survivors;             // per block of adaptive_fold_kernel: survivors, then their exclusive prefix sums
    DevBuf<uint32_t> d_n_active;            // [0] what the compaction counted
    int cur = 0;
    uint32_t n_active = 0, passes = 0;
    const void* last_preview = nullptr;     // the buffer the last pass wrote (the preview rule, adaptive.hpp)
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
    RAYZ_TRY(check_render_args(s, cam, p, p->precision)); // (either precision: the step entry must then match it)
    const uint64_t shard_pixels = (uint64_t)rayz_hip_shard_rows(p) * p->width;
    RAYZ_TRY(check_items(shard_pixels, 1));
    DeviceCtx* ctx = nullptr;
    RAYZ_TRY(scene_ctx(s->device, &ctx));
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
    if (e != hipSuccess) return hip_fail(e, "progressive handle");
    *out = pr.release();
    return RAYZ_OK;
}

template <class R>
int progressive_step(RayzProgressive* pr, uint32_t min_samples, R* d_preview, void* stream_arg, uint32_t precision) {
    typedef typename VecOf<R>::type r4;
    if (!pr) return fail(RAYZ_ERR_STATE, "progressive handle is null");
    if (pr->params.precision != precision)
        return fail(RAYZ_ERR_BAD_ARG, "params.precision %u does not match this entry point", pr->params.precision);
    if (pr->adaptive) return fail(RAYZ_ERR_STATE, "the handle is in adaptive mode: step it with rayz_hip_progressive_adaptive_step");
    const uint32_t n = (uint32_t)pr->starts.size() - 1, c0 = pr->chunks_done;
    if (c0 >= n) return fail(RAYZ_ERR_STATE, "the progressive render is finished (%u of %u chunks done)", c0, n);
    // the fewest whole chunks from the cursor that add at least min_samples samples (at least one, at most the rest)
    const uint64_t want = (uint64_t)pr->starts[c0] + min_samples;
    uint32_t c1 = (uint32_t)(std::lower_bound(pr->starts.begin() + c0 + 1, pr->starts.end(), want) - pr->starts.begin());
    if (c1 > n) c1 = n;
    RayzScene* s = pr->scene;
    DeviceCtx* ctx = nullptr;
    hipStream_t stream = nullptr;
    RAYZ_TRY(scene_stream(s->device, stream_arg, ctx, stream));
    DeviceScope scope(s->device);
    SceneBuffers<R>& b = buffers_of<R>(*s);
    bool use_bvh = false;
    RAYZ_TRY(prepare_scene<R>(s, b, &pr->cam, &pr->params, stream, use_bvh));
    RAYZ_TRY(check_items(pr->shard_pixels, c1 - c0));
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
        const int rc = trace_window<R>(s, *ctx, b, &pr->cam, &pr->params, use_bvh, pr->starts, pr->d_starts, c0, c1, pr->counters,
                                       sizeof(unsigned long long), ev0, ev1, stream, experiment, nullptr, 0, &pr->primary);
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
        RAYZ_TRY(read_counters(*pr->scene, pr->counters, "trace_kernel_bvh", pr->bvh, true, st, nothing_to_inspect));
        for (size_t i = 0; i + 1 < pr->pending.size(); i += 2) {
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, pr->pending[i], pr->pending[i + 1]));
            pr->kernel_ms += ms;
        }
        for (DevEvent& e : pr->pending) pr->spare.push_back(std::move(e));
        pr->pending.clear();
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
        return hip_fail(e, "noise state");
    }
    pr->tracked = true;
    return RAYZ_OK;
}

// Launches noise_eval_kernel on `stream` and, with `summary`, waits for it and fills the summary.  `acc`, `q`: `pixels` records.
template <class R>
int noise_eval(const void* acc, const d4* q, float* d_var, float* d_rel2, double* d_var64, double* d_rel264, unsigned long long* d_summary,
               double* d_block_sum, uint64_t pixels, uint32_t chunks_done, uint32_t samples_done, double floor2, double tau2,
               RayzNoiseSummary* summary, hipStream_t stream, const uint32_t* frozen_at = nullptr, const uint32_t* d_starts = nullptr) {
    typedef typename VecOf<R>::type r4;
    const uint32_t blocks = noise_blocks(pixels);
    if (pixels) {
        HIP_TRY(hipMemsetAsync(d_summary, 0, 2 * sizeof(unsigned long long), stream));
        if (frozen_at) // an adaptive handle: every pixel with its own (K_i, N_i)
            hipLaunchKernelGGL(noise_eval_adaptive_kernel<R>, dim3(blocks), dim3(256), 0, stream, (const r4*)acc, q, d_var, d_rel2, d_var64,
                               d_rel264, d_summary, d_block_sum, (uint32_t)pixels, chunks_done, samples_done, floor2, tau2, frozen_at, d_starts);
        else
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
    RAYZ_TRY(noise_params(params, tau2, floor2));
    if (!pr) return fail(RAYZ_ERR_STATE, "progressive handle is null");
    if (!pr->tracked) return fail(RAYZ_ERR_STATE, "the handle does not track noise (rayz_hip_progressive_track_noise before the first step)");
    DeviceCtx* ctx = nullptr;
    hipStream_t stream = nullptr;
    RAYZ_TRY(scene_stream(pr->scene->device, stream_arg, ctx, stream));
    DeviceScope scope(pr->device);
    if (pr->noise_stream && pr->noise_stream != stream) HIP_TRY(hipStreamSynchronize(pr->noise_stream)); // one evaluation owns the summary
    if (pr->last_stream && pr->last_stream != stream && pr->shard_pixels) HIP_TRY(hipStreamWaitEvent(stream, pr->pass_done, 0));
    pr->noise_stream = stream;
    const uint32_t K = pr->chunks_done, N = pr->starts[K];
    const uint32_t* frozen_at = pr->adaptive ? pr->frozen_at.get() : nullptr; // (the summary's cursor stays the schedule's)
    if (pr->params.precision == RAYZ_PRECISION_F64)
        return noise_eval<double>(pr->acc.get(), pr->q, d_var, d_rel2, nullptr, nullptr, pr->nz_summary, pr->nz_block_sum, pr->shard_pixels, K,
                                  N, floor2, tau2, summary, stream, frozen_at, pr->d_starts);
    return noise_eval<float>(pr->acc.get(), pr->q, d_var, d_rel2, nullptr, nullptr, pr->nz_summary, pr->nz_block_sum, pr->shard_pixels, K, N,
                             floor2, tau2, summary, stream, frozen_at, pr->d_starts);
}

// The per-channel variance of the mean (noise_rgb_kernel): ordered and owned as an evaluation is, without a summary.
int progressive_noise_rgb(RayzProgressive* pr, float* d_var_rgb, void* stream_arg) {
    if (!pr) return fail(RAYZ_ERR_STATE, "progressive handle is null");
    if (!pr->tracked) return fail(RAYZ_ERR_STATE, "the handle does not track noise (rayz_hip_progressive_track_noise before the first step)");
    if (!pr->shard_pixels) return RAYZ_OK;
    if (!d_var_rgb) return fail(RAYZ_ERR_BAD_ARG, "null buffer");
    DeviceCtx* ctx = nullptr;
    hipStream_t stream = nullptr;
    RAYZ_TRY(scene_stream(pr->scene->device, stream_arg, ctx, stream));
    DeviceScope scope(pr->device);
    if (pr->noise_stream && pr->noise_stream != stream) HIP_TRY(hipStreamSynchronize(pr->noise_stream));
    if (pr->last_stream && pr->last_stream != stream) HIP_TRY(hipStreamWaitEvent(stream, pr->pass_done, 0));
    pr->noise_stream = stream; // (a reader of acc and q, as an evaluation is)
    const uint32_t K = pr->chunks_done, N = pr->starts[K];
    const dim3 grid(noise_blocks(pr->shard_pixels)), block(256);
    if (pr->adaptive && pr->params.precision == RAYZ_PRECISION_F64)
        hipLaunchKernelGGL(noise_rgb_adaptive_kernel<double>, grid, block, 0, stream, (const VecOf<double>::type*)pr->acc.get(), (const d4*)pr->q,
                           d_var_rgb, (uint32_t)pr->shard_pixels, K, N, pr->frozen_at.get(), pr->d_starts.get());
    else if (pr->adaptive)
        hipLaunchKernelGGL(noise_rgb_adaptive_kernel<float>, grid, block, 0, stream, (const VecOf<float>::type*)pr->acc.get(), (const d4*)pr->q,
                           d_var_rgb, (uint32_t)pr->shard_pixels, K, N, pr->frozen_at.get(), pr->d_starts.get());
    else if (pr->params.precision == RAYZ_PRECISION_F64)
        hipLaunchKernelGGL(noise_rgb_kernel<double>, grid, block, 0, stream, (const VecOf<double>::type*)pr->acc.get(), (const d4*)pr->q, d_var_rgb,
                           (uint32_t)pr->shard_pixels, K, N);
    else
        hipLaunchKernelGGL(noise_rgb_kernel<float>, grid, block, 0, stream, (const VecOf<float>::type*)pr->acc.get(), (const d4*)pr->q, d_var_rgb,
                           (uint32_t)pr->shard_pixels, K, N);
    HIP_TRY(hipGetLastError());
    return RAYZ_OK;
}

int progressive_noise_state(RayzProgressive* pr, double* d_q, void* stream_arg) {
    if (!pr) return fail(RAYZ_ERR_STATE, "progressive handle is null");
    if (!pr->tracked) return fail(RAYZ_ERR_STATE, "the handle does not track noise (rayz_hip_progressive_track_noise before the first step)");
    if (!pr->shard_pixels) return RAYZ_OK;
    if (!d_q) return fail(RAYZ_ERR_BAD_ARG, "null buffer");
    DeviceCtx* ctx = nullptr;
    hipStream_t stream = nullptr;
    RAYZ_TRY(scene_stream(pr->scene->device, stream_arg, ctx, stream));
    DeviceScope scope(pr->device);
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
    RAYZ_TRY(noise_params(params, tau2, floor2));
    if (!(max_fraction >= 0.0 && max_fraction <= 1.0))
        return fail(RAYZ_ERR_BAD_ARG, "max_unconverged_fraction %g: must lie in [0, 1]", max_fraction);
    if (!pr) return fail(RAYZ_ERR_STATE, "progressive handle is null");
    if (!pr->tracked) return fail(RAYZ_ERR_STATE, "the handle does not track noise (rayz_hip_progressive_track_noise before the first step)");
    if (pr->adaptive) return fail(RAYZ_ERR_STATE, "the handle is in adaptive mode: run it with rayz_hip_progressive_run_adaptive");
    const uint32_t n = (uint32_t)pr->starts.size() - 1;
    RayzNoiseSummary sm{};
    for (;;) {
        RAYZ_TRY(progressive_step<R>(pr, min_samples, d_preview, stream_arg, precision));
        RAYZ_TRY(progressive_noise(pr, params, nullptr, nullptr, &sm, stream_arg));
        if ((double)sm.unconverged <= max_fraction * (double)sm.pixels || pr->chunks_done >= n) break;
    }
    if (last) *last = sm;
    return RAYZ_OK;
}

} // namespace

extern "C" {

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

int rayz_hip_progressive_noise_rgb(RayzProgressive* pr, float* d_var_rgb, void* stream) {
    return guarded([&] { return progressive_noise_rgb(pr, d_var_rgb, stream); });
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
int rayz_hip_progressive_destroy(RayzProgressive* pr) {
    return guarded([&] { return progressive_free(pr); });
}

} // extern "C"
