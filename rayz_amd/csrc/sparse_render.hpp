// sparse_render.hpp — sparse renders (rayz_hip_scene_render_pixels[_f64]): DESIGN.md §4.21; kernels: sparse.hpp.  Included by
// rayz_hip.hip; of the renderer it needs the scene, prepare_scene, the chunk schedule and the trace launch (trace_window with an
// active list, as an adaptive pass uses it).
#pragma once

namespace {

// Every argument is checked before a device is looked for, and every list entry (sparse_check_kernel) before anything is traced
// or written.  The one wait of the call is for that kernel's 4-byte count.
template <class R>
int scene_render_pixels(RayzScene* s, const RayzCameraDesc* cam, const RayzRenderParams* p, const uint32_t* d_pixels, uint32_t n_pixels,
                        const uint32_t* d_dest, uint32_t dest_pixels, R* d_out, float* d_var, void* stream_arg, uint32_t precision) {
    typedef typename VecOf<R>::type r4;
    RAYZ_TRY(check_render_args(s, cam, p, precision));
    if (!d_dest && dest_pixels != n_pixels)
        return fail(RAYZ_ERR_BAD_ARG, "sparse render: dest_pixels %u, but without d_dest entry j writes slot j of %u", dest_pixels, n_pixels);
    if (d_dest && n_pixels && !dest_pixels) return fail(RAYZ_ERR_BAD_ARG, "sparse render: d_dest names slots of an output of 0 pixels");
    if (!n_pixels) return RAYZ_OK;
    if (!d_pixels) return fail(RAYZ_ERR_BAD_ARG, "sparse render: the pixel list is null");
    if (!d_out) return fail(RAYZ_ERR_BAD_ARG, "sparse render: output pointer is null");
    const ShardGeometry shard = shard_geometry(p);
    const uint64_t shard_pixels64 = (uint64_t)shard.rows * p->width;
    RAYZ_TRY(check_items(shard_pixels64, 1));
    RAYZ_TRY(check_items(n_pixels, chunk_count(p)));

    DeviceCtx* ctx = nullptr;
    hipStream_t stream = nullptr;
    RAYZ_TRY(scene_stream(s->device, stream_arg, ctx, stream));
    DeviceScope scope(s->device);
    SceneBuffers<R>& b = buffers_of<R>(*s);
    bool use_bvh = false;
    RAYZ_TRY(prepare_scene<R>(s, b, cam, p, stream, use_bvh)); // (waits for a render the scene has in flight on another stream)
    std::vector<uint32_t> starts;
    chunk_schedule(p, starts);
    const uint32_t chunks = (uint32_t)starts.size() - 1;
    if (!s->sparse_bad) HIP_TRY(s->sparse_bad.alloc(1));
    if (!s->counters) HIP_TRY(s->counters.alloc(32));
    if (!s->sparse_ev[0])
        for (DevEvent& e : s->sparse_ev) HIP_TRY(e.create());
    RAYZ_TRY(scene_schedule(s, starts, stream));

    const dim3 grid((n_pixels + 255u) / 256u), block(256);
    HIP_TRY(hipMemsetAsync(s->sparse_bad, 0, sizeof(uint32_t), stream));
    HIP_TRY(hipEventRecord(s->sparse_ev[0], stream));
    hipLaunchKernelGGL(sparse_check_kernel, grid, block, 0, stream, d_pixels, d_dest, n_pixels, (uint32_t)shard_pixels64, dest_pixels,
                       s->sparse_bad.get());
    HIP_TRY(hipGetLastError());
    uint32_t bad = 0;
    HIP_TRY(hipMemcpyAsync(&bad, s->sparse_bad, sizeof(bad), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (bad) {
        if (s->last_sparse) s->rendered = false; // (the events of the last sparse render are this call's now: nothing left to time)
        return fail(RAYZ_ERR_BAD_ARG, "sparse render: %u of %u entries name a pixel outside the shard's %llu or a slot outside the output's %u",
                    bad, n_pixels, (unsigned long long)shard_pixels64, d_dest ? dest_pixels : n_pixels);
    }

    s->last = RayzRenderStats{};
    s->last.primary_rays = (uint64_t)n_pixels * p->samples_per_px;
    s->last_bvh = use_bvh;
    s->last_experiment = 0;
    s->last_stream = stream;
    s->rendered = s->last_sparse = false; // (until the launches below are out: a failure among them leaves nothing to report)
    const bool black = p->max_bounces == 0; // bounceRay(ray, 0) is black: nothing to trace, every sum is +0
    if (!black) // (its own events stay inside the call's)
        RAYZ_TRY(trace_window<R>(s, *ctx, b, cam, p, use_bvh, starts, s->chunk_start, 0, chunks, s->counters, 32 * sizeof(unsigned long long),
                                 s->sparse_ev[2], s->sparse_ev[3], stream, s->last_experiment, d_pixels, n_pixels));
    if (d_var)
        hipLaunchKernelGGL((sparse_resolve_kernel<R, true>), grid, block, 0, stream, (const r4*)s->partial.get(), d_dest, n_pixels, d_out, d_var,
                           (const uint32_t*)s->chunk_start.get(), black ? 0u : chunks, chunks, p->samples_per_px);
    else
        hipLaunchKernelGGL((sparse_resolve_kernel<R, false>), grid, block, 0, stream, (const r4*)s->partial.get(), d_dest, n_pixels, d_out,
                           (float*)nullptr, (const uint32_t*)s->chunk_start.get(), black ? 0u : chunks, chunks, p->samples_per_px);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->sparse_ev[1], stream));
    s->rendered = !black;
    s->last_sparse = !black;
    return RAYZ_OK;
}

} // namespace

extern "C" {

int rayz_hip_scene_render_pixels(RayzScene* scene, const RayzCameraDesc* camera, const RayzRenderParams* params, const uint32_t* d_pixels,
                                 uint32_t n_pixels, const uint32_t* d_dest_or_null, uint32_t dest_pixels, float* d_rgb_out,
                                 float* d_var_rgb_out_or_null, void* hip_stream) {
    return guarded([&] {
        return scene_render_pixels<float>(scene, camera, params, d_pixels, n_pixels, d_dest_or_null, dest_pixels, d_rgb_out,
                                          d_var_rgb_out_or_null, hip_stream, RAYZ_PRECISION_F32);
    });
}

int rayz_hip_scene_render_pixels_f64(RayzScene* scene, const RayzCameraDesc* camera, const RayzRenderParams* params, const uint32_t* d_pixels,
                                     uint32_t n_pixels, const uint32_t* d_dest_or_null, uint32_t dest_pixels, double* d_rgb_out,
                                     float* d_var_rgb_out_or_null, void* hip_stream) {
    return guarded([&] {
        return scene_render_pixels<double>(scene, camera, params, d_pixels, n_pixels, d_dest_or_null, dest_pixels, d_rgb_out,
                                           d_var_rgb_out_or_null, hip_stream, RAYZ_PRECISION_F64);
    });
}

} // extern "C"
