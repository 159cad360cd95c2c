// sampled.hpp — sampled G-buffers (rayz_hip_scene_query_camera_sampled): the host side.  Kernels:
// sampled_kernel.hpp.  Included by rayz_hip.hip behind query.hpp and chain.hpp, whose checks, counters, events and sync it shares: a
// sampled call is the scene's query in flight, and rayz_hip_query_sync waits for it.
#pragma once

namespace {

template <class R>
int scene_query_camera_sampled(RayzScene* s, const RayzCameraDesc* cam, const RayzRenderParams* p, uint32_t samples,
                               const RayzSampledOutputs* out, void* stream_arg) {
    using namespace rayz_dev_sampled;
    const uint32_t rows = rayz_hip_shard_rows(p);
    const uint64_t pixels = (uint64_t)rows * p->width;
    if (pixels >= (1ull << 31)) return fail(RAYZ_ERR_BAD_ARG, "camera query of %llu pixels", (unsigned long long)pixels);
    if (pixels == 0) return RAYZ_OK;
    const uint32_t n = (uint32_t)pixels;
    DeviceCtx* pctx = nullptr;
    hipStream_t stream = nullptr;
    RAYZ_TRY(scene_stream(s->device, stream_arg, pctx, stream));
    DeviceScope scope(s->device);
    const DeviceCtx& ctx = *pctx;
    SceneBuffers<R>& b = buffers_of<R>(*s);
    if (s->last_stream && s->last_stream != stream) HIP_TRY(hipStreamSynchronize(s->last_stream)); // one launch in flight per scene
    if (!s->q_counters) {
        HIP_TRY(s->q_counters.alloc(kQueryCounterWords));
        HIP_TRY(hipMemset(s->q_counters, 0, kQueryCounterWords * sizeof(unsigned long long)));
    }
    if (!s->q_ev0) {
        HIP_TRY(s->q_ev0.create());
        HIP_TRY(s->q_ev1.create());
    }
    // the sums of a call of more than one sample: 8 R per pixel (a call still using a smaller workspace is waited for first)
    const size_t sum_bytes = samples > 1u ? (size_t)n * kSumWords * sizeof(R) : 0;
    if (sum_bytes > s->q_sampled_sums.capacity() || !s->q_sampled_sums) {
        if (s->last_stream) HIP_TRY(hipStreamSynchronize(s->last_stream));
        HIP_TRY(s->q_sampled_sums.alloc(sum_bytes));
    }
    bool use_bvh = false; // (camera_origin_bound covers the lens disk)
    RAYZ_TRY(prepare_scene_bound<R>(s, b, camera_origin_bound(cam), p->traversal, stream, use_bvh));

    SampledArgs<R> A{};
    A.q.sc = dev_scene<R>(*s, b, use_bvh);
    fill_camera<R>(cam, A.q.cam);
    A.q.rays = nullptr;
    A.q.tmin = (R)p->tmin;
    A.q.n = n;
    A.q.kind = RAYZ_QUERY_NEAREST;
    const ShardGeometry shard = shard_geometry(p);
    A.q.width = p->width;
    A.q.tile_rows = shard.tile_rows;
    A.q.shard_index = p->shard_index;
    A.q.shard_count = shard.shard_count;
    A.q.tiled_pixels = shard.tiled_pixels;
    A.q.counters = s->q_counters;
    A.samples = samples;
    SampledStores<R> stores{(R*)out->albedo, (R*)out->normal, (R*)out->t, out->hits, (R*)s->q_sampled_sums.get(), p->seed, p->samples_per_px};
    ChainStoreWords words{}; // (the chain call's way of handing a kernel its words, and its buffer)
    static_assert(sizeof(stores) == kSampledStoreWords * sizeof(unsigned long long) && kSampledStoreWords <= kChainStoreWords,
                  "a SampledStores is kSampledStoreWords words");
    std::memcpy(&words, &stores, sizeof(stores));
    if (!s->q_chain_stores) HIP_TRY(s->q_chain_stores.alloc(kChainStoreWords));
    A.out = (const SampledStores<R>*)s->q_chain_stores.get();

    typedef void (*Kernel)(const SampledArgs<R>);
    Kernel kernel = sampled_kernel<R>;
    int block = 256;
    BvhLds L;
    if (use_bvh) { // the render's LDS layout, as a query's
        kernel = b.quantized ? sampled_kernel_bvh<R, true> : sampled_kernel_bvh<R, false>;
        block = (int)kBvhWg;
        RAYZ_TRY(bvh_lds_layout(kernel, "sampled", block, bvh_stack_bytes(s->bvh_dev.depth, kBvhWg), b.quantized, b.n_big_leaves, b.bvh_top, 0, L));
        A.q.bvh_top_words = L.top_words;
        A.q.bvh_big_words = L.big_words;
        A.q.sc.bvh_top = L.top_bytes;
    }
    uint64_t grid = (n + (uint64_t)block - 1) / block;
    if (use_bvh) grid = std::min<uint64_t>(grid, (uint64_t)ctx.num_cu * std::max(1, L.blocks_per_cu));
    s->last_stream = stream;
    s->q_stream = stream;
    s->q_bvh = use_bvh;
    s->q_chain = false; // (the segments are known here: pixels · n)
    s->q_sampled = true;
    s->q_last = RayzRenderStats{};
    s->q_last.primary_rays = s->q_last.segments = (uint64_t)n * samples;
    HIP_TRY(hipMemsetAsync(s->q_counters, 0, 4 * sizeof(unsigned long long), stream));
    hipLaunchKernelGGL(chain_outputs_kernel, dim3(1), dim3(64), 0, stream, words, s->q_chain_stores.get()); // (behind the scene's last query)
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->q_ev0, stream));
    hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(block), L.lds, stream, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->q_ev1, stream));
    s->queried = true;
    return RAYZ_OK;
}

} // namespace

extern "C" {

int rayz_hip_scene_query_camera_sampled(RayzScene* s, const RayzCameraDesc* cam, const RayzRenderParams* p, const RayzSampledParams* sampled,
                                        const RayzSampledOutputs* out, void* stream) {
    // every argument is checked before the first HIP call
    if (!p) return fail(RAYZ_ERR_BAD_ARG, "params is null");
    RAYZ_TRY(check_query_args(s, RAYZ_QUERY_NEAREST, p->precision, p->traversal, p->tmin));
    if (!cam) return fail(RAYZ_ERR_BAD_ARG, "camera is null");
    if (!out) return fail(RAYZ_ERR_BAD_ARG, "outputs is null");
    if (!p->width || !p->height) return fail(RAYZ_ERR_BAD_ARG, "width and height must be > 0");
    const uint32_t sc = p->shard_count ? p->shard_count : 1;
    if (p->shard_index >= sc) return fail(RAYZ_ERR_BAD_ARG, "shard_index %u >= shard_count %u", p->shard_index, sc);
    if (!p->samples_per_px) return fail(RAYZ_ERR_BAD_ARG, "samples_per_px must be > 0 (it is the stride of the path ids)");
    const uint32_t samples = sampled && sampled->samples ? sampled->samples : p->samples_per_px;
    if (samples > p->samples_per_px)
        return fail(RAYZ_ERR_BAD_ARG, "samples %u > samples_per_px %u: the path ids would run into the next pixel's", samples, p->samples_per_px);
    return guarded([&] {
        return p->precision == RAYZ_PRECISION_F64 ? scene_query_camera_sampled<double>(s, cam, p, samples, out, stream)
                                                  : scene_query_camera_sampled<float>(s, cam, p, samples, out, stream);
    });
}

} // extern "C"
