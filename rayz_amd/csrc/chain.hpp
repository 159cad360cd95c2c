// chain.hpp — specular-chain G-buffers (rayz_hip_scene_query_camera_chain): the host side.  Kernels:
// chain_kernel.hpp.  Included by rayz_hip.hip behind query.hpp, whose checks, counters, events and sync it shares: a chain call
// is the scene's query in flight, and rayz_hip_query_sync waits for it.
#pragma once

namespace {

template <class R>
int scene_query_camera_chain(RayzScene* s, const RayzCameraDesc* cam, const RayzRenderParams* p, const RayzChainParams& ch,
                             const RayzQueryOutputs* out, const RayzChainOutputs* co, void* stream_arg) {
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
    // (every later segment starts at a hit point: inside the bound the scene's padding always covers, prepare_scene_bound)
    bool use_bvh = false;
    RAYZ_TRY(prepare_scene_bound<R>(s, b, camera_origin_bound(cam), p->traversal, stream, use_bvh));

    ChainArgs<R> A{};
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
    ChainStores<R> stores{out->index, (R*)out->t, (R*)out->point, (R*)out->normal, out->front_face, out->material, (R*)out->albedo,
                          out->hit, co ? co->key : nullptr, co ? co->depth : nullptr, co ? co->first_index : nullptr};
    ChainStoreWords words;
    static_assert(sizeof(stores) == sizeof(words), "a ChainStores is kChainStoreWords pointers");
    std::memcpy(&words, &stores, sizeof(words));
    if (!s->q_chain_stores) HIP_TRY(s->q_chain_stores.alloc(kChainStoreWords));
    A.out = (const ChainStores<R>*)s->q_chain_stores.get();
    A.max_fuzz = ch.max_fuzz;
    A.max_depth = ch.max_depth;

    typedef void (*Kernel)(const ChainArgs<R>);
    Kernel kernel = chain_kernel<R>;
    int block = 256;
    BvhLds L;
    if (use_bvh) { // the render's LDS layout, as a query's
        kernel = b.quantized ? chain_kernel_bvh<R, true> : chain_kernel_bvh<R, false>;
        block = (int)kBvhWg;
        RAYZ_TRY(bvh_lds_layout(kernel, "chain", block, bvh_stack_bytes(s->bvh_dev.depth, kBvhWg), b.quantized, b.n_big_leaves, b.bvh_top, 0, L));
        A.q.bvh_top_words = L.top_words;
        A.q.bvh_big_words = L.big_words;
        A.q.sc.bvh_top = L.top_bytes;
    }
    uint64_t grid = (n + (uint64_t)block - 1) / block;
    if (use_bvh) grid = std::min<uint64_t>(grid, (uint64_t)ctx.num_cu * std::max(1, L.blocks_per_cu));
    s->last_stream = stream;
    s->q_stream = stream;
    s->q_bvh = use_bvh;
    s->q_chain = true;
    s->q_last = RayzRenderStats{};
    s->q_last.primary_rays = n;
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

int rayz_hip_scene_query_camera_chain(RayzScene* s, const RayzCameraDesc* cam, const RayzRenderParams* p, const RayzChainParams* chain,
                                      const RayzQueryOutputs* out, const RayzChainOutputs* chain_out, void* stream) {
    // every argument is checked before the first HIP call
    if (!p) return fail(RAYZ_ERR_BAD_ARG, "params is null");
    RAYZ_TRY(check_query_args(s, RAYZ_QUERY_NEAREST, p->precision, p->traversal, p->tmin));
    if (!cam) return fail(RAYZ_ERR_BAD_ARG, "camera is null");
    if (!out) return fail(RAYZ_ERR_BAD_ARG, "outputs is null");
    if (!p->width || !p->height) return fail(RAYZ_ERR_BAD_ARG, "width and height must be > 0");
    const uint32_t sc = p->shard_count ? p->shard_count : 1;
    if (p->shard_index >= sc) return fail(RAYZ_ERR_BAD_ARG, "shard_index %u >= shard_count %u", p->shard_index, sc);
    const RayzChainParams ch = chain ? *chain : RayzChainParams{RAYZ_CHAIN_DEFAULT_DEPTH, 0, RAYZ_CHAIN_DEFAULT_MAX_FUZZ};
    if (ch.max_depth > RAYZ_CHAIN_MAX_DEPTH) return fail(RAYZ_ERR_BAD_ARG, "chain max_depth %u > %u", ch.max_depth, RAYZ_CHAIN_MAX_DEPTH);
    if (!(ch.max_fuzz >= 0.0)) return fail(RAYZ_ERR_BAD_ARG, "chain max_fuzz %g: must not be negative or NaN", ch.max_fuzz);
    return guarded([&] {
        return p->precision == RAYZ_PRECISION_F64 ? scene_query_camera_chain<double>(s, cam, p, ch, out, chain_out, stream)
                                                  : scene_query_camera_chain<float>(s, cam, p, ch, out, chain_out, stream);
    });
}

} // extern "C"
