// query.hpp — ray queries on a device scene (rayz_hip_scene_query*): nearest hit, any hit and G-buffers.  Included by
// rayz_hip.hip, behind what it shares with the trace launch (prepare_scene_bound, dev_scene, bvh_lds_layout, shard_geometry, read_counters).
#pragma once

namespace {

// query_key (query_kernel.hpp) and its inverse on the host: an order-preserving u64 of a double
unsigned long long query_key_host(double x) {
    unsigned long long b;
    std::memcpy(&b, &x, 8);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
double query_unkey_host(unsigned long long k) {
    const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    double x;
    std::memcpy(&x, &b, 8);
    return x;
}

// What every query entry checks before touching a device.
int check_query_args(RayzScene* s, uint32_t kind, uint32_t precision, uint32_t traversal, double tmin) {
    if (!s) return fail(RAYZ_ERR_BAD_ARG, "scene handle is null");
    if (kind > RAYZ_QUERY_ANY) return fail(RAYZ_ERR_BAD_ARG, "bad query kind %u", kind);
    if (precision > RAYZ_PRECISION_F64) return fail(RAYZ_ERR_BAD_ARG, "bad precision %u", precision);
    if (traversal > RAYZ_TRAVERSAL_AUTO) return fail(RAYZ_ERR_BAD_ARG, "bad traversal %u", traversal);
    if (!(tmin == tmin)) return fail(RAYZ_ERR_BAD_ARG, "tmin is NaN");
    return RAYZ_OK;
}

// The bound check of a batch: max |origin|, time range and refusals (query_bounds_kernel), read back — the one wait of a query.
constexpr uint32_t kQueryBoundBase = 32, kQueryCounterWords = kQueryBoundBase + 4 * kQueryBoundStride;
template <class R> int query_bounds(RayzScene* s, const DeviceCtx& ctx, const R* rays, uint32_t n, hipStream_t stream, double& S) {
    unsigned long long init[4 * kQueryBoundStride] = {};
    init[0] = query_key_host(0.0);
    init[kQueryBoundStride] = query_key_host(std::numeric_limits<double>::infinity());
    init[2 * kQueryBoundStride] = query_key_host(-std::numeric_limits<double>::infinity());
    unsigned long long* words = s->q_counters.get() + kQueryBoundBase;
    HIP_TRY(hipMemcpyAsync(words, init, sizeof(init), hipMemcpyHostToDevice, stream));
    const uint32_t blocks = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)ctx.num_cu * 2, (n + 255) / 256));
    hipLaunchKernelGGL(query_bounds_kernel<R>, dim3(blocks), dim3(256), 0, stream, rays, n, words);
    HIP_TRY(hipGetLastError());
    unsigned long long got[4 * kQueryBoundStride] = {};
    HIP_TRY(hipMemcpyAsync(got, words, sizeof(got), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const unsigned long long flags = got[3 * kQueryBoundStride];
    if (flags & 1u) return fail(RAYZ_ERR_BAD_ARG, "query rays: a NaN or infinite origin, direction or time");
    if (flags & 8u) return fail(RAYZ_ERR_BAD_ARG, "query rays: an origin component beyond RAYZ_QUERY_MAX_ORIGIN (%g)", (double)RAYZ_QUERY_MAX_ORIGIN);
    if (flags & 2u) return fail(RAYZ_ERR_BAD_ARG, "query rays: a zero direction");
    if (flags & 16u)
        return fail(RAYZ_ERR_BAD_ARG, "query rays: a direction whose largest component lies outside [2^-32, 2^32] "
                                      "(RAYZ_QUERY_MIN_DIR, RAYZ_QUERY_MAX_DIR)");
    if (flags & 4u) return fail(RAYZ_ERR_BAD_ARG, "query rays: a NaN tmax");
    const double tlo = query_unkey_host(got[kQueryBoundStride]), thi = query_unkey_host(got[2 * kQueryBoundStride]);
    if (tlo < 0.0 || thi > 1.0)
        return fail(RAYZ_ERR_BAD_ARG, "query rays: time %g outside [0, 1] (the BVH's moving-sphere boxes cover [0, 1] only)",
                    tlo < 0.0 ? tlo : thi);
    S = query_unkey_host(got[0]) * (1.0 + 1e-6); // (the norm is rounded in f64: a relative margin far above its error)
    return RAYZ_OK;
}

// One query launch: rays (or the camera form when rays == NULL, `cam` / `p` then describe it) on the scene's device and its stream.
template <class R>
int query_impl(RayzScene* s, uint32_t kind, uint32_t traversal, double tmin, uint32_t n, const R* rays, const RayzCameraDesc* cam,
               const RayzRenderParams* p, const RayzQueryOutputs* out, void* stream_arg) {
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
    double S = 0;
    if (rays) RAYZ_TRY(query_bounds<R>(s, ctx, rays, n, stream, S));
    else S = camera_origin_bound(cam);
    bool use_bvh = false;
    RAYZ_TRY(prepare_scene_bound<R>(s, b, S, traversal, stream, use_bvh));

    QueryArgs<R> A{};
    A.sc = dev_scene<R>(*s, b, use_bvh);
    if (cam) fill_camera<R>(cam, A.cam);
    A.rays = rays;
    A.tmin = (R)tmin;
    A.n = n;
    A.kind = kind;
    if (!rays) {
        const ShardGeometry shard = shard_geometry(p);
        A.width = p->width;
        A.tile_rows = shard.tile_rows;
        A.shard_index = p->shard_index;
        A.shard_count = shard.shard_count;
        A.tiled_pixels = shard.tiled_pixels;
    }
    A.counters = s->q_counters;
    A.index = out->index;
    A.t = (R*)out->t;
    A.point = (R*)out->point;
    A.normal = (R*)out->normal;
    A.front = out->front_face;
    A.material = out->material;
    A.albedo = (R*)out->albedo;
    A.hit = out->hit;

    typedef void (*Kernel)(const QueryArgs<R>);
    Kernel kernel = query_kernel<R>;
    int block = 256;
    BvhLds L;
    if (use_bvh) { // the render's LDS layout, with nothing extra behind it (RAYZ_DEBUG_LDS_PAD is the trace launch's alone)
        kernel = b.quantized ? query_kernel_bvh<R, true> : query_kernel_bvh<R, false>;
        block = (int)kBvhWg;
        RAYZ_TRY(bvh_lds_layout(kernel, "query", block, bvh_stack_bytes(s->bvh_dev.depth, kBvhWg), b.quantized, b.n_big_leaves, b.bvh_top, 0, L));
        A.bvh_top_words = L.top_words;
        A.bvh_big_words = L.big_words;
        A.sc.bvh_top = L.top_bytes;
    }
    uint64_t grid = (n + (uint64_t)block - 1) / block;
    if (use_bvh) grid = std::min<uint64_t>(grid, (uint64_t)ctx.num_cu * std::max(1, L.blocks_per_cu));
    s->last_stream = stream;
    s->q_stream = stream;
    s->q_bvh = use_bvh;
    s->q_chain = false;
    s->q_sampled = false;
    s->q_last = RayzRenderStats{};
    s->q_last.primary_rays = s->q_last.segments = n;
    HIP_TRY(hipMemsetAsync(s->q_counters, 0, 4 * sizeof(unsigned long long), stream));
    HIP_TRY(hipEventRecord(s->q_ev0, stream));
    hipLaunchKernelGGL(kernel, dim3((uint32_t)grid), dim3(block), L.lds, stream, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(s->q_ev1, stream));
    s->queried = true;
    return RAYZ_OK;
}

template <class R>
int scene_query(RayzScene* s, const RayzQueryParams* q, const void* rays, const RayzQueryOutputs* out, void* stream_arg) {
    if (!q) return fail(RAYZ_ERR_BAD_ARG, "query params is null");
    return query_impl<R>(s, q->kind, q->traversal, q->tmin, q->n_rays, (const R*)rays, nullptr, nullptr, out, stream_arg);
}

template <class R>
int scene_query_camera(RayzScene* s, const RayzCameraDesc* cam, const RayzRenderParams* p, const RayzQueryOutputs* out,
                       void* stream_arg) {
    const uint32_t rows = rayz_hip_shard_rows(p);
    const uint64_t pixels = (uint64_t)rows * p->width;
    if (pixels >= (1ull << 31)) return fail(RAYZ_ERR_BAD_ARG, "camera query of %llu pixels", (unsigned long long)pixels);
    if (pixels == 0) return RAYZ_OK;
    return query_impl<R>(s, RAYZ_QUERY_NEAREST, p->traversal, p->tmin, (uint32_t)pixels, nullptr, cam, p, out, stream_arg);
}

int query_sync(RayzScene* s, RayzRenderStats* stats) {
    if (!s) return fail(RAYZ_ERR_BAD_ARG, "scene handle is null");
    if (!s->queried) {
        if (stats) *stats = s->q_last;
        return RAYZ_OK;
    }
    DeviceScope scope(s->device);
    HIP_TRY(hipStreamSynchronize(s->q_stream));
    RayzRenderStats st = s->q_last; // (its segments: the batch's rays, query_impl; a chain call's: counted by its kernel, chain.hpp)
    RAYZ_TRY(read_counters(*s, s->q_counters, s->q_chain ? "chain_kernel_bvh" : s->q_sampled ? "sampled_kernel_bvh" : "query_kernel_bvh", s->q_bvh, s->q_chain, st, nothing_to_inspect));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, s->q_ev0, s->q_ev1));
    st.kernel_ms = ms;
    s->q_last = st;
    s->queried = false;
    if (stats) *stats = s->q_last;
    return RAYZ_OK;
}

} // namespace

extern "C" {

int rayz_hip_scene_query(RayzScene* s, const RayzQueryParams* q, const void* d_rays, const RayzQueryOutputs* out, void* stream) {
    // every argument is checked before the first HIP call
    if (!q) return fail(RAYZ_ERR_BAD_ARG, "query params is null");
    RAYZ_TRY(check_query_args(s, q->kind, q->precision, q->traversal, q->tmin));
    if (!out) return fail(RAYZ_ERR_BAD_ARG, "outputs is null");
    if (q->n_rays == 0) return RAYZ_OK;
    if (!d_rays) return fail(RAYZ_ERR_BAD_ARG, "rays is null");
    return guarded([&] {
        return q->precision == RAYZ_PRECISION_F64 ? scene_query<double>(s, q, d_rays, out, stream)
                                                  : scene_query<float>(s, q, d_rays, out, stream);
    });
}

int rayz_hip_scene_query_camera(RayzScene* s, const RayzCameraDesc* cam, const RayzRenderParams* p, const RayzQueryOutputs* out,
                                void* stream) {
    if (!p) return fail(RAYZ_ERR_BAD_ARG, "params is null");
    RAYZ_TRY(check_query_args(s, RAYZ_QUERY_NEAREST, p->precision, p->traversal, p->tmin));
    if (!cam) return fail(RAYZ_ERR_BAD_ARG, "camera is null");
    if (!out) return fail(RAYZ_ERR_BAD_ARG, "outputs is null");
    if (!p->width || !p->height) return fail(RAYZ_ERR_BAD_ARG, "width and height must be > 0");
    const uint32_t sc = p->shard_count ? p->shard_count : 1;
    if (p->shard_index >= sc) return fail(RAYZ_ERR_BAD_ARG, "shard_index %u >= shard_count %u", p->shard_index, sc);
    return guarded([&] {
        return p->precision == RAYZ_PRECISION_F64 ? scene_query_camera<double>(s, cam, p, out, stream)
                                                  : scene_query_camera<float>(s, cam, p, out, stream);
    });
}

int rayz_hip_query_sync(RayzScene* s, RayzRenderStats* stats) {
    return guarded([&] { return query_sync(s, stats); });
}

} // extern "C"
