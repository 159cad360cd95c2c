// adaptive_passes.hpp — adaptive passes (rayz_hip_progressive_set_adaptive, _adaptive_step, _run_adaptive, _sample_counts,
// _frozen_at, rayz_hip_adaptive_kat): DESIGN.md §4.14; kernels: adaptive.hpp.  Included by rayz_hip.hip, behind progressive.hpp
// (the handle, noise_params, progressive_track_noise) and the trace launch (trace_window with an active list).
#pragma once

namespace {

uint32_t adaptive_blocks(uint64_t entries) { return (uint32_t)((entries + 255) / 256); }

// Allocates frozen_at (cleared), both lists, the survivor counts and the counter for `pixels` pixels, and deals the first list
// (adaptive_list_init_kernel) on `stream`.
int adaptive_alloc(DevBuf<uint32_t>& frozen_at, DevBuf<uint32_t> (&lists)[2], DevBuf<uint32_t>& survivors, DevBuf<uint32_t>& d_n_active,
                   uint64_t pixels, uint32_t tiled_pixels, uint32_t width, hipStream_t stream) {
    hipError_t e = frozen_at.alloc(pixels);
    if (e == hipSuccess) e = lists[0].alloc(pixels);
    if (e == hipSuccess) e = lists[1].alloc(pixels);
    if (e == hipSuccess) e = survivors.alloc(adaptive_blocks(pixels));
    if (e == hipSuccess) e = d_n_active.alloc(1);
    if (e == hipSuccess && pixels) e = hipMemsetAsync(frozen_at, 0, pixels * sizeof(uint32_t), stream);
    if (e != hipSuccess) return hip_fail(e, "adaptive state");
    if (pixels) {
        hipLaunchKernelGGL(adaptive_list_init_kernel, dim3(adaptive_blocks(pixels)), dim3(256), 0, stream, lists[0].get(), (uint32_t)pixels,
                           tiled_pixels, width);
        HIP_TRY(hipGetLastError());
    }
    return RAYZ_OK;
}

// Fold, freeze and compact one pass on `stream`: `partial` holds the `chunks` compact chunk sums of list's n_active entries (the
// chunks [c1 - chunks, c1) of the schedule `d_starts`; chunks = 0 folds nothing).  Leaves the next list in `next` and waits for
// its length, which replaces n_active.
template <class R>
int adaptive_fold_compact(const void* partial, const uint32_t* list, uint32_t* next, uint32_t& n_active, void* acc, d4* q,
                          uint32_t* frozen_at, R* out, const uint32_t* d_starts, uint32_t chunks, uint32_t c1, uint32_t samples_end,
                          uint32_t min_chunks, double floor2, double tau2, uint32_t* survivors, uint32_t* d_n_active, hipStream_t stream) {
    typedef typename VecOf<R>::type r4;
    if (!n_active) return RAYZ_OK;
    const uint32_t blocks = adaptive_blocks(n_active);
    hipLaunchKernelGGL(adaptive_fold_kernel<R>, dim3(blocks), dim3(256), 0, stream, (const r4*)partial, list, n_active, (r4*)acc, q, frozen_at,
                       out, d_starts + (c1 - chunks), chunks, c1, samples_end, min_chunks, floor2, tau2, survivors);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(adaptive_scan_kernel, dim3(1), dim3(1024), 0, stream, survivors, blocks, d_n_active);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(adaptive_scatter_kernel, dim3(blocks), dim3(256), 0, stream, list, n_active, (const uint32_t*)frozen_at,
                       (const uint32_t*)survivors, next);
    HIP_TRY(hipGetLastError());
    uint32_t left = 0;
    HIP_TRY(hipMemcpyAsync(&left, d_n_active, sizeof(left), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (left > n_active) return fail(RAYZ_ERR_STATE, "adaptive compaction counted %u survivors of %u entries", left, n_active);
    n_active = left;
    return RAYZ_OK;
}

int progressive_set_adaptive(RayzProgressive* pr, uint32_t min_chunks) {
    if (min_chunks < 2) return fail(RAYZ_ERR_BAD_ARG, "min_chunks %u: at least 2 (there is no estimate before the second chunk)", min_chunks);
    if (!pr) return fail(RAYZ_ERR_STATE, "progressive handle is null");
    if (pr->chunks_done || pr->passes) return fail(RAYZ_ERR_STATE, "adaptive mode starts before the first step (%u chunks done)", pr->chunks_done);
    if (pr->adaptive) {
        pr->min_chunks = min_chunks;
        return RAYZ_OK;
    }
    // The adaptive state first, tracking second: a failure of either leaves the handle the plain one it was (buffers allocated here
    // are unused until `adaptive` is set, and a later call allocates them anew).
    {
        DeviceCtx* ctx = nullptr;
        RAYZ_TRY(scene_ctx(pr->scene->device, &ctx));
        DeviceScope scope(pr->device);
        const ShardGeometry shard = shard_geometry(&pr->params);
        RAYZ_TRY(adaptive_alloc(pr->frozen_at, pr->active, pr->survivors, pr->d_n_active, pr->shard_pixels, shard.tiled_pixels,
                                pr->params.width, ctx->stream));
        HIP_TRY(hipStreamSynchronize(ctx->stream));
    }
    RAYZ_TRY(progressive_track_noise(pr));
    pr->adaptive = true;
    pr->min_chunks = min_chunks;
    pr->cur = 0;
    pr->n_active = (uint32_t)pr->shard_pixels;
    return RAYZ_OK;
}

void adaptive_summary(const RayzProgressive* pr, RayzAdaptiveSummary* out) {
    if (!out) return;
    RayzAdaptiveSummary sm{};
    sm.pixels = pr->shard_pixels, sm.active = pr->n_active, sm.samples_traced = pr->primary_rays;
    sm.passes = pr->passes, sm.chunks_done = pr->chunks_done, sm.samples_done = pr->starts[pr->chunks_done];
    *out = sm;
}

bool adaptive_finished(const RayzProgressive* pr) { return !pr->n_active || pr->chunks_done >= (uint32_t)pr->starts.size() - 1; }

template <class R>
int progressive_adaptive_step(RayzProgressive* pr, const RayzNoiseParams* params, uint32_t min_samples, R* d_preview,
                              RayzAdaptiveSummary* summary, void* stream_arg, uint32_t precision) {
    typedef typename VecOf<R>::type r4;
    double tau2 = 0, floor2 = 0;
    RAYZ_TRY(noise_params(params, tau2, floor2));
    if (!pr) return fail(RAYZ_ERR_STATE, "progressive handle is null");
    if (!pr->adaptive) return fail(RAYZ_ERR_STATE, "the handle is not in adaptive mode (rayz_hip_progressive_set_adaptive before the first step)");
    if (pr->params.precision != precision)
        return fail(RAYZ_ERR_BAD_ARG, "params.precision %u does not match this entry point", pr->params.precision);
    RayzScene* s = pr->scene;
    DeviceCtx* ctx = nullptr;
    hipStream_t stream = nullptr;
    RAYZ_TRY(scene_stream(s->device, stream_arg, ctx, stream));
    DeviceScope scope(s->device);
    const dim3 px_grid(adaptive_blocks(pr->shard_pixels)), block(256);
    auto whole_frame = [&]() -> int { // (chunks_done >= 1 wherever a pixel exists: see below)
        hipLaunchKernelGGL(adaptive_frame_kernel<R>, px_grid, block, 0, stream, (const r4*)pr->acc.get(), (const uint32_t*)pr->frozen_at.get(),
                           (const uint32_t*)pr->d_starts.get(), pr->chunks_done, d_preview, (uint32_t)pr->shard_pixels);
        HIP_TRY(hipGetLastError());
        return RAYZ_OK;
    };
    if (adaptive_finished(pr)) { // nothing to trace: the frame on request
        if (d_preview && pr->shard_pixels && pr->chunks_done) {
            if (pr->last_stream && pr->last_stream != stream) HIP_TRY(hipStreamSynchronize(pr->last_stream));
            RAYZ_TRY(whole_frame());
            HIP_TRY(hipStreamSynchronize(stream));
            pr->last_preview = d_preview;
        }
        adaptive_summary(pr, summary);
        return RAYZ_OK;
    }
    const uint32_t n = (uint32_t)pr->starts.size() - 1, c0 = pr->chunks_done;
    const uint64_t want = (uint64_t)pr->starts[c0] + min_samples; // rayz_hip_progressive_step's window
    uint32_t c1 = (uint32_t)(std::lower_bound(pr->starts.begin() + c0 + 1, pr->starts.end(), want) - pr->starts.begin());
    if (c1 > n) c1 = n;
    SceneBuffers<R>& b = buffers_of<R>(*s);
    bool use_bvh = false;
    RAYZ_TRY(prepare_scene<R>(s, b, &pr->cam, &pr->params, stream, use_bvh));
    RAYZ_TRY(check_items(pr->n_active, c1 - c0));
    if (pr->last_stream && pr->last_stream != stream) HIP_TRY(hipStreamSynchronize(pr->last_stream)); // the accumulator's last pass
    if (pr->noise_stream && pr->noise_stream != stream) HIP_TRY(hipStreamSynchronize(pr->noise_stream)); // .. and its last reader
    pr->bvh = use_bvh;
    const uint64_t samples = pr->starts[c1] - pr->starts[c0];
    const uint32_t traced = pr->n_active;
    const bool black = pr->params.max_bounces == 0; // bounceRay(ray, 0) is black: nothing to trace, the sums are +0 (acc and Q stay so)
    const uint32_t* list = pr->active[pr->cur].get();
    if (!black) {
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
        int experiment = 0;
        const int rc = trace_window<R>(s, *ctx, b, &pr->cam, &pr->params, use_bvh, pr->starts, pr->d_starts, c0, c1, pr->counters,
                                       sizeof(unsigned long long), ev0, ev1, stream, experiment, list, traced);
        if (rc != RAYZ_OK) {
            pr->spare.push_back(std::move(ev0));
            pr->spare.push_back(std::move(ev1));
            return rc;
        }
        pr->pending.push_back(std::move(ev0));
        pr->pending.push_back(std::move(ev1));
        pr->traced = true;
    }
    pr->last_stream = stream;
    // the preview rule (adaptive.hpp): the pass's own pixels into the buffer the last pass wrote, every pixel into another one
    const bool whole = d_preview && d_preview != pr->last_preview;
    RAYZ_TRY(adaptive_fold_compact<R>(s->partial.get(), list, pr->active[pr->cur ^ 1].get(), pr->n_active, pr->acc.get(), pr->q.get(),
                                      pr->frozen_at.get(), whole ? (R*)nullptr : d_preview, pr->d_starts.get(), black ? 0u : c1 - c0, c1,
                                      pr->starts[c1], pr->min_chunks, floor2, tau2, pr->survivors.get(), pr->d_n_active.get(), stream));
    pr->cur ^= 1;
    pr->chunks_done = c1;
    pr->primary_rays += (uint64_t)traced * samples;
    pr->passes++;
    if (whole) RAYZ_TRY(whole_frame());
    pr->last_preview = d_preview; // (a pass without a buffer wrote none: the next pass with one writes every pixel)
    HIP_TRY(hipEventRecord(pr->pass_done, stream));
    if (whole) HIP_TRY(hipStreamSynchronize(stream));
    adaptive_summary(pr, summary);
    return RAYZ_OK;
}

template <class R>
int progressive_run_adaptive(RayzProgressive* pr, const RayzNoiseParams* params, uint32_t min_samples, R* d_preview,
                             RayzAdaptiveSummary* last, void* stream_arg, uint32_t precision) {
    RayzAdaptiveSummary sm{};
    do { // (the step refuses a null handle before adaptive_finished reads it)
        RAYZ_TRY(progressive_adaptive_step<R>(pr, params, min_samples, d_preview, &sm, stream_arg, precision));
    } while (!adaptive_finished(pr));
    if (last) *last = sm;
    return RAYZ_OK;
}

// sample_counts (counts = true) and frozen_at: ordered and owned as an evaluation is; block.
int progressive_adaptive_read(RayzProgressive* pr, uint32_t* d_out, bool counts, void* stream_arg) {
    if (!pr) return fail(RAYZ_ERR_STATE, "progressive handle is null");
    if (!pr->adaptive) return fail(RAYZ_ERR_STATE, "the handle is not in adaptive mode (rayz_hip_progressive_set_adaptive before the first step)");
    if (!pr->shard_pixels) return RAYZ_OK;
    if (!d_out) return fail(RAYZ_ERR_BAD_ARG, "null buffer");
    DeviceCtx* ctx = nullptr;
    hipStream_t stream = nullptr;
    RAYZ_TRY(scene_stream(pr->scene->device, stream_arg, ctx, stream));
    DeviceScope scope(pr->device);
    if (pr->last_stream && pr->last_stream != stream) HIP_TRY(hipStreamSynchronize(pr->last_stream));
    if (counts) {
        hipLaunchKernelGGL(adaptive_counts_kernel, dim3(adaptive_blocks(pr->shard_pixels)), dim3(256), 0, stream,
                           (const uint32_t*)pr->frozen_at.get(), (const uint32_t*)pr->d_starts.get(), pr->chunks_done, d_out,
                           (uint32_t)pr->shard_pixels);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemcpyAsync(d_out, pr->frozen_at, pr->shard_pixels * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    return RAYZ_OK;
}

int adaptive_kat(uint32_t precision, const double* sums, const uint32_t* sizes, uint32_t n_pixels, uint32_t n_chunks, const uint32_t* pass_ends,
                 uint32_t n_passes, uint32_t width, uint32_t min_chunks, const RayzNoiseParams* params, uint32_t* frozen_at_out, double* acc_out,
                 double* q_out, double* frame_out, uint32_t* lists_out, uint32_t* list_sizes_out) {
    double tau2 = 0, floor2 = 0;
    RAYZ_TRY(noise_params(params, tau2, floor2));
    if (precision > RAYZ_PRECISION_F64) return fail(RAYZ_ERR_BAD_ARG, "bad precision %u", precision);
    if (min_chunks < 2) return fail(RAYZ_ERR_BAD_ARG, "min_chunks %u: at least 2 (there is no estimate before the second chunk)", min_chunks);
    if (!n_chunks || !n_passes) return fail(RAYZ_ERR_BAD_ARG, "n_chunks or n_passes is 0");
    if (!sizes || !pass_ends || (n_pixels && !sums)) return fail(RAYZ_ERR_BAD_ARG, "null buffer");
    if ((uint64_t)n_pixels * n_chunks > (1ull << 28)) return fail(RAYZ_ERR_BAD_ARG, "n_pixels x n_chunks = %llu: more than 2^28 chunk sums",
                                                                   (unsigned long long)n_pixels * n_chunks);
    if (width && n_pixels % width) return fail(RAYZ_ERR_BAD_ARG, "n_pixels %u is not whole rows of width %u", n_pixels, width);
    std::vector<uint32_t> starts(n_chunks + 1, 0);
    for (uint32_t k = 0; k < n_chunks; ++k) {
        if (!sizes[k] || (uint64_t)starts[k] + sizes[k] > UINT32_MAX)
            return fail(RAYZ_ERR_BAD_ARG, "chunk_sizes[%u] = %u: a chunk holds at least one sample, and all of them at most 2^32 - 1", k, sizes[k]);
        starts[k + 1] = starts[k] + sizes[k];
    }
    for (uint32_t p = 0; p < n_passes; ++p)
        if (pass_ends[p] > n_chunks || pass_ends[p] <= (p ? pass_ends[p - 1] : 0u))
            return fail(RAYZ_ERR_BAD_ARG, "pass_ends[%u] = %u: strictly increasing chunk counts in 1 .. n_chunks", p, pass_ends[p]);
    int device;
    hipStream_t stream;
    RAYZ_TRY(default_device(device, stream));
    if (list_sizes_out) std::fill(list_sizes_out, list_sizes_out + n_passes + 1, 0u);
    if (!n_pixels) return RAYZ_OK;
    const bool f64 = precision == RAYZ_PRECISION_F64;
    const size_t r4_bytes = f64 ? sizeof(d4) : sizeof(f4);
    const uint32_t tiled_pixels = width && width % 8 == 0 ? n_pixels / width / 8 * 8 * width : 0u;
    DeviceScope scope(device);
    DevBytes d_partial, d_acc, d_frame;
    DevBuf<d4> d_q;
    DevBuf<uint32_t> d_starts, frozen_at, lists[2], survivors, d_n_active;
    hipError_t e = d_acc.alloc(n_pixels * r4_bytes);
    if (e == hipSuccess) e = d_q.alloc(n_pixels);
    if (e == hipSuccess) e = d_frame.alloc((size_t)n_pixels * 3 * (f64 ? sizeof(double) : sizeof(float)));
    if (e == hipSuccess) e = d_starts.upload(starts);
    if (e == hipSuccess) e = hipMemsetAsync(d_acc, 0, n_pixels * r4_bytes, stream);
    if (e == hipSuccess) e = hipMemsetAsync(d_q, 0, n_pixels * sizeof(d4), stream);
    if (e != hipSuccess) return hip_fail(e, "rayz_hip_adaptive_kat");
    RAYZ_TRY(adaptive_alloc(frozen_at, lists, survivors, d_n_active, n_pixels, tiled_pixels, width, stream));
    uint32_t n_active = n_pixels, c0 = 0, done = 0;
    int cur = 0;
    std::vector<uint32_t> list(n_pixels);
    std::vector<char> host;
    auto report = [&](uint32_t p) -> int { // list p, as the pass about to run reads it
        HIP_TRY(hipStreamSynchronize(stream));
        if (n_active) HIP_TRY(hipMemcpy(list.data(), lists[cur], n_active * sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (lists_out) std::copy(list.begin(), list.begin() + n_active, lists_out + (size_t)p * n_pixels);
        if (list_sizes_out) list_sizes_out[p] = n_active;
        return RAYZ_OK;
    };
    for (uint32_t p = 0; p < n_passes && n_active; ++p) {
        RAYZ_TRY(report(p));
        for (uint32_t j = 0; j < n_active; ++j)
            if (list[j] >= n_pixels) return fail(RAYZ_ERR_STATE, "active list %u entry %u = %u: outside the %u pixels", p, j, list[j], n_pixels);
        const uint32_t c1 = pass_ends[p], chunks = c1 - c0;
        host.assign((size_t)chunks * n_active * r4_bytes, 0); // the compact chunk sums a trace pass over this list would have left
        for (uint32_t k = 0; k < chunks; ++k)
            for (uint32_t j = 0; j < n_active; ++j) {
                const double* v = sums + ((size_t)(c0 + k) * n_pixels + list[j]) * 3;
                const size_t at = (size_t)k * n_active + j;
                if (f64) reinterpret_cast<d4*>(host.data())[at] = d4{v[0], v[1], v[2], 0.0};
                else reinterpret_cast<f4*>(host.data())[at] = f4{(float)v[0], (float)v[1], (float)v[2], 0.0f};
            }
        if (host.size() > d_partial.capacity()) HIP_TRY(d_partial.alloc(host.size())); // (the stream is idle: report waited)
        HIP_TRY(hipMemcpy(d_partial, host.data(), host.size(), hipMemcpyHostToDevice));
        if (f64)
            RAYZ_TRY(adaptive_fold_compact<double>(d_partial.get(), lists[cur], lists[cur ^ 1], n_active, d_acc.get(), d_q, frozen_at, nullptr,
                                                   d_starts, chunks, c1, starts[c1], min_chunks, floor2, tau2, survivors, d_n_active, stream));
        else
            RAYZ_TRY(adaptive_fold_compact<float>(d_partial.get(), lists[cur], lists[cur ^ 1], n_active, d_acc.get(), d_q, frozen_at, nullptr,
                                                  d_starts, chunks, c1, starts[c1], min_chunks, floor2, tau2, survivors, d_n_active, stream));
        cur ^= 1, c0 = c1, done = p + 1;
    }
    RAYZ_TRY(report(done));
    // (passes after the last pixel froze trace nothing: their lists stay empty)
    const dim3 grid(adaptive_blocks(n_pixels)), block(256);
    if (f64)
        hipLaunchKernelGGL(adaptive_frame_kernel<double>, grid, block, 0, stream, (const d4*)d_acc.get(), (const uint32_t*)frozen_at,
                           (const uint32_t*)d_starts, c0, (double*)d_frame.get(), n_pixels);
    else
        hipLaunchKernelGGL(adaptive_frame_kernel<float>, grid, block, 0, stream, (const f4*)d_acc.get(), (const uint32_t*)frozen_at,
                           (const uint32_t*)d_starts, c0, (float*)d_frame.get(), n_pixels);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(stream));
    if (frozen_at_out) HIP_TRY(hipMemcpy(frozen_at_out, frozen_at, n_pixels * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (q_out) {
        std::vector<d4> q(n_pixels);
        HIP_TRY(hipMemcpy(q.data(), d_q, n_pixels * sizeof(d4), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n_pixels; ++i) q_out[3 * i] = q[i].x, q_out[3 * i + 1] = q[i].y, q_out[3 * i + 2] = q[i].z;
    }
    if (acc_out) {
        host.resize(n_pixels * r4_bytes);
        HIP_TRY(hipMemcpy(host.data(), d_acc, host.size(), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n_pixels; ++i)
            for (int ch = 0; ch < 3; ++ch)
                acc_out[3 * i + ch] = f64 ? reinterpret_cast<const double*>(host.data())[4 * (size_t)i + ch]
                                          : (double)reinterpret_cast<const float*>(host.data())[4 * (size_t)i + ch];
    }
    if (frame_out) {
        host.resize((size_t)n_pixels * 3 * (f64 ? sizeof(double) : sizeof(float)));
        HIP_TRY(hipMemcpy(host.data(), d_frame, host.size(), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < (size_t)n_pixels * 3; ++i)
            frame_out[i] = f64 ? reinterpret_cast<const double*>(host.data())[i] : (double)reinterpret_cast<const float*>(host.data())[i];
    }
    return RAYZ_OK;
}

} // namespace

extern "C" {

int rayz_hip_progressive_set_adaptive(RayzProgressive* pr, uint32_t min_chunks) {
    return guarded([&] { return progressive_set_adaptive(pr, min_chunks); });
}

int rayz_hip_progressive_adaptive_step(RayzProgressive* pr, const RayzNoiseParams* p, uint32_t min_samples, float* d_preview,
                                       RayzAdaptiveSummary* summary, void* stream) {
    return guarded([&] { return progressive_adaptive_step<float>(pr, p, min_samples, d_preview, summary, stream, RAYZ_PRECISION_F32); });
}

int rayz_hip_progressive_adaptive_step_f64(RayzProgressive* pr, const RayzNoiseParams* p, uint32_t min_samples, double* d_preview,
                                           RayzAdaptiveSummary* summary, void* stream) {
    return guarded([&] { return progressive_adaptive_step<double>(pr, p, min_samples, d_preview, summary, stream, RAYZ_PRECISION_F64); });
}

int rayz_hip_progressive_run_adaptive(RayzProgressive* pr, const RayzNoiseParams* p, uint32_t min_samples_per_pass, float* d_preview,
                                      RayzAdaptiveSummary* last, void* stream) {
    return guarded([&] { return progressive_run_adaptive<float>(pr, p, min_samples_per_pass, d_preview, last, stream, RAYZ_PRECISION_F32); });
}

int rayz_hip_progressive_run_adaptive_f64(RayzProgressive* pr, const RayzNoiseParams* p, uint32_t min_samples_per_pass, double* d_preview,
                                          RayzAdaptiveSummary* last, void* stream) {
    return guarded([&] { return progressive_run_adaptive<double>(pr, p, min_samples_per_pass, d_preview, last, stream, RAYZ_PRECISION_F64); });
}

int rayz_hip_progressive_sample_counts(RayzProgressive* pr, uint32_t* d_counts, void* stream) {
    return guarded([&] { return progressive_adaptive_read(pr, d_counts, true, stream); });
}

int rayz_hip_progressive_frozen_at(RayzProgressive* pr, uint32_t* d_frozen_at, void* stream) {
    return guarded([&] { return progressive_adaptive_read(pr, d_frozen_at, false, stream); });
}

int rayz_hip_adaptive_kat(uint32_t precision, const double* chunk_sums, const uint32_t* chunk_sizes, uint32_t n_pixels, uint32_t n_chunks,
                          const uint32_t* pass_ends, uint32_t n_passes, uint32_t width, uint32_t min_chunks, const RayzNoiseParams* p,
                          uint32_t* frozen_at_out, double* acc_out, double* q_out, double* frame_out, uint32_t* lists_out,
                          uint32_t* list_sizes_out) {
    return guarded([&] {
        return adaptive_kat(precision, chunk_sums, chunk_sizes, n_pixels, n_chunks, pass_ends, n_passes, width, min_chunks, p, frozen_at_out,
                            acc_out, q_out, frame_out, lists_out, list_sizes_out);
    });
}

} // extern "C"
