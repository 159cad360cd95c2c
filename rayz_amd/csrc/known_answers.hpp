// known_answers.hpp — the known-answer entries: rayz_hip_kat runs the trace kernels' device functions on caller inputs, rayz_hip_noise_kat
// the noise estimate's fold and evaluation on caller chunk sums.  Included by rayz_hip.hip, behind progressive.hpp (noise_params, noise_eval).
#pragma once

namespace {

int noise_kat(uint32_t precision, const double* sums, const uint32_t* sizes, uint32_t n_pixels, uint32_t n_chunks,
              const RayzNoiseParams* params, double* q_out, double* var_out, double* rel2_out, RayzNoiseSummary* summary) {
    double tau2 = 0, floor2 = 0;
    RAYZ_TRY(noise_params(params, tau2, floor2));
    if (precision > RAYZ_PRECISION_F64) return fail(RAYZ_ERR_BAD_ARG, "bad precision %u", precision);
    if (!n_chunks) return fail(RAYZ_ERR_BAD_ARG, "n_chunks is 0");
    if (!sizes || (n_pixels && !sums)) return fail(RAYZ_ERR_BAD_ARG, "null buffer");
    if ((uint64_t)n_pixels * n_chunks > (1ull << 28)) return fail(RAYZ_ERR_BAD_ARG, "n_pixels x n_chunks = %llu: more than 2^28 chunk sums",
                                                                   (unsigned long long)n_pixels * n_chunks);
    std::vector<uint32_t> starts(n_chunks + 1, 0);
    for (uint32_t k = 0; k < n_chunks; ++k) {
        if (!sizes[k] || (uint64_t)starts[k] + sizes[k] > UINT32_MAX)
            return fail(RAYZ_ERR_BAD_ARG, "chunk_sizes[%u] = %u: a chunk holds at least one sample, and all of them at most 2^32 - 1", k, sizes[k]);
        starts[k + 1] = starts[k] + sizes[k];
    }
    int device;
    hipStream_t stream;
    RAYZ_TRY(default_device(device, stream));
    if (!n_pixels) {
        if (summary) *summary = RayzNoiseSummary{0, 0, 0.0, 0.0, starts[n_chunks], n_chunks};
        return RAYZ_OK;
    }
    const bool f64 = precision == RAYZ_PRECISION_F64;
    const size_t items = (size_t)n_pixels * n_chunks, r4_bytes = f64 ? sizeof(d4) : sizeof(f4);
    std::vector<char> host(items * r4_bytes); // the chunk-sum records a trace pass would have left
    for (size_t i = 0; i < items; ++i) {
        if (f64) reinterpret_cast<d4*>(host.data())[i] = d4{sums[3 * i], sums[3 * i + 1], sums[3 * i + 2], 0.0};
        else reinterpret_cast<f4*>(host.data())[i] = f4{(float)sums[3 * i], (float)sums[3 * i + 1], (float)sums[3 * i + 2], 0.0f};
    }
    DeviceScope scope(device);
    DevBytes d_partial, d_acc;
    DevBuf<d4> d_q;
    DevBuf<uint32_t> d_starts;
    DevBuf<double> d_var, d_rel2, d_block_sum;
    DevBuf<unsigned long long> d_summary;
    const uint32_t blocks = noise_blocks(n_pixels);
    hipError_t e = d_partial.alloc(host.size());
    if (e == hipSuccess) e = d_acc.alloc(n_pixels * r4_bytes);
    if (e == hipSuccess) e = d_q.alloc(n_pixels);
    if (e == hipSuccess) e = d_starts.upload(starts);
    if (e == hipSuccess) e = d_var.alloc(n_pixels);
    if (e == hipSuccess) e = d_rel2.alloc(n_pixels);
    if (e == hipSuccess) e = d_block_sum.alloc(blocks);
    if (e == hipSuccess) e = d_summary.alloc(2);
    if (e == hipSuccess) e = hipMemcpyAsync(d_partial, host.data(), host.size(), hipMemcpyHostToDevice, stream);
    if (e != hipSuccess) return hip_fail(e, "rayz_hip_noise_kat");
    // the fold as two passes: chunk 0 from +0, then the rest onto acc and q
    for (uint32_t pass = 0; pass < (n_chunks > 1 ? 2u : 1u); ++pass) {
        const uint32_t c0 = pass, c1 = pass ? n_chunks : 1;
        const char* src = d_partial.get() + (size_t)c0 * n_pixels * r4_bytes;
        if (f64)
            hipLaunchKernelGGL(accumulate_moments_kernel<double>, dim3(blocks), dim3(256), 0, stream, (const d4*)src, (d4*)d_acc.get(), d_q.get(),
                               (double*)nullptr, d_starts.get() + c0, n_pixels, c1 - c0, starts[c1], pass ? 0u : 1u);
        else
            hipLaunchKernelGGL(accumulate_moments_kernel<float>, dim3(blocks), dim3(256), 0, stream, (const f4*)src, (f4*)d_acc.get(), d_q.get(),
                               (float*)nullptr, d_starts.get() + c0, n_pixels, c1 - c0, starts[c1], pass ? 0u : 1u);
        HIP_TRY(hipGetLastError());
    }
    RayzNoiseSummary sm{};
    RAYZ_TRY(f64 ? noise_eval<double>(d_acc.get(), d_q, nullptr, nullptr, d_var, d_rel2, d_summary, d_block_sum, n_pixels, n_chunks, starts[n_chunks],
                                  floor2, tau2, &sm, stream)
             : noise_eval<float>(d_acc.get(), d_q, nullptr, nullptr, d_var, d_rel2, d_summary, d_block_sum, n_pixels, n_chunks, starts[n_chunks],
                                 floor2, tau2, &sm, stream)); // (noise_eval has waited for the stream)
    if (q_out) {
        std::vector<d4> q(n_pixels);
        HIP_TRY(hipMemcpy(q.data(), d_q, n_pixels * sizeof(d4), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < n_pixels; ++i) q_out[3 * i] = q[i].x, q_out[3 * i + 1] = q[i].y, q_out[3 * i + 2] = q[i].z;
    }
    if (var_out) HIP_TRY(hipMemcpy(var_out, d_var, n_pixels * sizeof(double), hipMemcpyDeviceToHost));
    if (rel2_out) HIP_TRY(hipMemcpy(rel2_out, d_rel2, n_pixels * sizeof(double), hipMemcpyDeviceToHost));
    if (summary) *summary = sm;
    return RAYZ_OK;
}

} // namespace

extern "C" {

int rayz_hip_noise_kat(uint32_t precision, const double* chunk_sums, const uint32_t* chunk_sizes, uint32_t n_pixels, uint32_t n_chunks,
                       const RayzNoiseParams* p, double* q_out, double* var_out, double* rel2_out, RayzNoiseSummary* summary) {
    return guarded([&] { return noise_kat(precision, chunk_sums, chunk_sizes, n_pixels, n_chunks, p, q_out, var_out, rel2_out, summary); });
}

// ---- known answers: the kernel's device functions on caller inputs ---------------------------------------------
int rayz_hip_kat(uint32_t op, uint32_t precision, const double* in, uint32_t n, double* out) {
    return guarded([&] {
        if (op > RAYZ_KAT_SET_DISCS) return fail(RAYZ_ERR_BAD_ARG, "bad known-answer op %u", op);
        if (precision > RAYZ_PRECISION_F64) return fail(RAYZ_ERR_BAD_ARG, "bad precision %u", precision);
        if (!n) return (int)RAYZ_OK;
        if (!in || !out) return fail(RAYZ_ERR_BAD_ARG, "null buffer");
        int device;
        hipStream_t stream;
        RAYZ_TRY(default_device(device, stream));
        std::vector<double> host(in, in + (size_t)n * RAYZ_KAT_IN_STRIDE);
        for (uint32_t i = 0; i < n; ++i) { // what the scene upload would have prepared for these hittables
            double* a = host.data() + (size_t)i * RAYZ_KAT_IN_STRIDE;
            // the list of uniforms must lie inside the record: the device reads u[0 .. n_u)
            if (op == RAYZ_KAT_GET_RAY || op == RAYZ_KAT_SCATTER) {
                const int at = op == RAYZ_KAT_GET_RAY ? 21 : 16;
                const double nu = a[at];
                const bool no_rng = op == RAYZ_KAT_GET_RAY && nu == -1.0; // getRay(px, py, null)
                if (!no_rng && !(nu >= 0 && nu <= RAYZ_KAT_IN_STRIDE - (at + 1) && nu == std::floor(nu)))
                    return fail(RAYZ_ERR_BAD_ARG, "record %u: n_u = %g is not an integer in [0, %d]%s", i, nu, RAYZ_KAT_IN_STRIDE - (at + 1),
                                op == RAYZ_KAT_GET_RAY ? " (or -1: no generator)" : "");
            }
            if (op == RAYZ_KAT_BOX_HIT) { // the box as a scene upload would hold it (S = this ray's origin, B = this box), in the format a[26] names
                rayz_bvh::Box bx;
                double B = 0;
                for (int k = 0; k < 3; ++k) bx.lo[k] = a[k], bx.hi[k] = a[3 + k], B = std::max({B, std::fabs(a[k]), std::fabs(a[3 + k])});
                if (a[26] != 0.0) { // f32 planes
                    const double pad = kBoxPadUlps * unit_roundoff<float>() * std::max(norm3(a + 6), B);
                    for (int k = 0; k < 3; ++k) {
                        a[14 + k] = (double)rayz_bvh::roundDown<float>(bx.lo[k] - pad), a[17 + k] = (double)rayz_bvh::roundUp<float>(bx.hi[k] + pad);
                        a[20 + k] = 0.0, a[23 + k] = 1.0;
                    }
                } else { // 16-bit plane indices on the grid over this box
                    double pad = kBoxPadUlps * unit_roundoff<float>() * (std::max(norm3(a + 6), B) + 2.0 * B);
                    const rayz_bvh::PlaneGrid g = rayz_bvh::PlaneGrid::over(bx.lo, bx.hi, 2.0 * pad);
                    pad = kBoxPadUlps * unit_roundoff<float>() * (std::max(norm3(a + 6), B) + g.extent);
                    uint32_t w[3];
                    g.quantize(bx, pad, w);
                    for (int k = 0; k < 3; ++k) a[14 + k] = w[k] & 0xffffu, a[17 + k] = w[k] >> 16, a[20 + k] = g.glo[k], a[23 + k] = g.cell[k];
                }
            }
            if (op == RAYZ_KAT_SCAN_DISCS || op == RAYZ_KAT_SCAN_DISCS_XY) { // the padded squares the scan streams would hold for these four spheres
                const double cls = a[27];
                if (!(cls == 0.0 || cls == 1.0 || cls == 2.0 || cls == 3.0))
                    return fail(RAYZ_ERR_BAD_ARG, "record %u: class = %g is not 0, 1, 2 or 3", i, cls);
                if (!(a[32] == 0.0 || a[32] == 1.0)) return fail(RAYZ_ERR_BAD_ARG, "record %u: want_r2 = %g is not 0 or 1", i, a[32]);
                if (cls >= 2.0) { // a plane run: one f32 height, bit for bit (+0 and -0 are two runs), as plan_runs groups them
                    const uint32_t h = rayz_plane::bits32((float)a[4]);
                    for (int k = 1; k < 4; ++k)
                        if (rayz_plane::bits32((float)a[4 + k]) != h)
                            return fail(RAYZ_ERR_BAD_ARG, "record %u: plane-run class %g with cy[%d] = %.9g != cy[0] = %.9g in f32", i, cls, k,
                                        (double)(float)a[4 + k], (double)(float)a[4]);
                }
                double S = norm3(a + 20);
                RayzSphere q[4] = {};
                for (int k = 0; k < 4; ++k) {
                    q[k].center[0] = a[k], q[k].center[1] = a[4 + k], q[k].center[2] = a[8 + k];
                    q[k].radius = a[12 + k];
                    q[k].velocity[1] = cls == 1.0 || cls == 3.0 ? a[16 + k] : 0.0;
                    S = std::max(S, norm3(q[k].center) + norm3(q[k].velocity) + std::fabs(q[k].radius));
                }
                for (int k = 0; k < 4; ++k)
                    a[28 + k] = precision == RAYZ_PRECISION_F32 ? (double)pad_radius2_scan<float>(q[k], S) : (double)pad_radius2_scan<double>(q[k], S);
            }
            if (op == RAYZ_KAT_BUCKET_DISCS || op == RAYZ_KAT_BUCKET_DISCS_XY) { // the padded squares a speed bucket of speed v0 would hold for these four spheres
                if (!std::isfinite(a[27])) return fail(RAYZ_ERR_BAD_ARG, "record %u: v0 = %g is not finite", i, a[27]);
                double S = norm3(a + 20);
                RayzSphere q[4] = {};
                for (int k = 0; k < 4; ++k) {
                    q[k].center[0] = a[k], q[k].center[1] = a[4], q[k].center[2] = a[8 + k];
                    q[k].radius = a[12 + k];
                    q[k].velocity[1] = a[16 + k];
                    S = std::max(S, norm3(q[k].center) + norm3(q[k].velocity) + std::fabs(q[k].radius));
                }
                for (int k = 0; k < 4; ++k)
                    a[28 + k] = precision == RAYZ_PRECISION_F32 ? (double)pad_radius2_bucket<float>(q[k], S, (float)a[27])
                                                                : (double)pad_radius2_bucket<double>(q[k], S, (float)a[27]);
            }
            if (op == RAYZ_KAT_SET_DISCS) { // the padded square a one-radius set of radius Rp would hold for these eight members
                if (!std::isfinite(a[17])) return fail(RAYZ_ERR_BAD_ARG, "record %u: v0 = %g is not finite", i, a[17]);
                if (!(a[19] == 0.0 || a[19] == 1.0)) return fail(RAYZ_ERR_BAD_ARG, "record %u: movy = %g is not 0 or 1", i, a[19]);
                if (!(a[18] >= 0.0 && std::isfinite(a[18]))) return fail(RAYZ_ERR_BAD_ARG, "record %u: Rp = %g is not a finite radius", i, a[18]);
                double S = norm3(a + 20);
                RayzSphere q[8] = {};
                for (int k = 0; k < 8; ++k) {
                    q[k].center[0] = a[k], q[k].center[1] = a[16], q[k].center[2] = a[8 + k];
                    q[k].velocity[1] = a[19] != 0.0 ? a[28 + k] : 0.0;
                    S = std::max(S, norm3(q[k].center) + norm3(q[k].velocity) + a[18]);
                }
                float R2 = 0.0f;
                for (int k = 0; k < 8; ++k) {
                    const double h = a[19] != 0.0 ? rayz_plane::bucket_h(q[k].velocity[1], (float)a[17]) : 0.0;
                    R2 = std::max(R2, rayz_plane::pad_radius2_set(q[k].center, q[k].velocity, S, h, a[18], precision != RAYZ_PRECISION_F32));
                }
                a[36] = (double)R2;
            }
            if (op == RAYZ_KAT_SPHERE_HIT) {
                RayzSphere q{};
                for (int k = 0; k < 3; ++k) q.center[k] = a[k], q.velocity[k] = a[3 + k];
                q.radius = a[6];
                const double S = std::max(norm3(a + 7), norm3(q.center) + norm3(q.velocity) + std::fabs(q.radius));
                a[16] = precision == RAYZ_PRECISION_F32 ? (double)pad_radius2_scan<float>(q, S) : (double)pad_radius2_scan<double>(q, S);
            }
        }
        DeviceScope scope(device);
        DevBuf<double> d_in, d_out;
        const size_t in_bytes = host.size() * sizeof(double), out_bytes = (size_t)n * RAYZ_KAT_OUT_STRIDE * sizeof(double);
        hipError_t e = d_in.alloc(host.size());
        if (e == hipSuccess) e = d_out.alloc((size_t)n * RAYZ_KAT_OUT_STRIDE);
        if (e == hipSuccess) e = hipMemcpyAsync(d_in, host.data(), in_bytes, hipMemcpyHostToDevice, stream);
        if (e == hipSuccess) {
            if (precision == RAYZ_PRECISION_F32) hipLaunchKernelGGL(kat_kernel<float>, dim3((n + 63) / 64), dim3(64), 0, stream, op, d_in.get(), n, d_out.get());
            else hipLaunchKernelGGL(kat_kernel<double>, dim3((n + 63) / 64), dim3(64), 0, stream, op, d_in.get(), n, d_out.get());
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return hip_fail(e, "rayz_hip_kat");
        return (int)RAYZ_OK;
    });
}

} // extern "C"
