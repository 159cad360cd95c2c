// trace_kernel_flat.hpp — the text of the persistent flat-list trace kernel (described in rayz_device.hpp, which includes this file
// FOUR times: as trace_kernel, the product kernel, as flat_xy_kernel — RAYZ_TRACE_KERNEL_BASIS kBasisXY — the same kernel with
// the reject test's other basis, as flat_one_radius_kernel — RAYZ_TRACE_KERNEL_SETS true — that one with the one-radius sets in a
// loop of their own, and — RAYZ_TRACE_KERNEL_ADAPTIVE true — as adaptive_pass_kernel, the kernel of an
// adaptive pass).  One text, four kernels of four NAMES, and not further template flags on trace_kernel:
// tests/test_isa_invariants.py counts the kernels named trace_kernel.. (six) and holds each to the product's limits, so a kernel
// of that name is a product kernel; the adaptive ones are held to the same limits by tests/test_adaptive_isa.py.  Nor a shared
// body FUNCTION: handing the kernel's argument block to it changes the product kernel's register allocation; compiled twice,
// trace_kernel's ISA is what it was.  No include guard.
// RAYZ_TRACE_KERNEL_PRIMARY true — three more times, as primary_xz_kernel, primary_xy_kernel and primary_one_radius_kernel: the
// three scan forms with each path's CAMERA segment resolved from its pixel's primary list (primary_lists.hpp)
// instead of a scan.  An iteration of the loop is then either a LIST phase — taken while any lane of the wave holds a fresh path
// (seg == 0) on a pixel that has a list: those lanes alone take their listed slots through narrow_eval, count the segment and
// shade; a path that ends there (sky, absorption, depth) is replaced at the top of the next iteration, the chunk retired and the
// next item popped as ever — or a SCAN phase as before, once every live lane's next segment needs the scan (a later segment,
// or the camera segment of a pixel without a list).  The refill therefore repeats, wave-cooperative, until every lane holds a
// path that needs a scan or the queue is drained; nothing else differs: same streams, same sums, same segments counter.
#ifdef RAYZ_TRACE_KERNEL_ARGS
template <class R, int NR> __global__ __launch_bounds__(256, (flat_waves<R, NR>())) void RAYZ_TRACE_KERNEL_NAME(const RAYZ_TRACE_KERNEL_ARGS A) {
#else
template <class R, int NR> __global__ __launch_bounds__(256, (flat_waves<R, NR>())) void RAYZ_TRACE_KERNEL_NAME(const TraceArgs<R> A) {
#endif
    constexpr bool kAdaptive = RAYZ_TRACE_KERNEL_ADAPTIVE; // work items over the active list (place_item)
#ifdef RAYZ_TRACE_KERNEL_BASIS
    constexpr int kBasis = RAYZ_TRACE_KERNEL_BASIS; // the reject test's basis (RayBasis)
#else
    constexpr int kBasis = kBasisXZ;
#endif
#ifdef RAYZ_TRACE_KERNEL_SETS
    constexpr bool kSets = RAYZ_TRACE_KERNEL_SETS; // the one-radius sets in their own loop (scan_plane_class)
#else
    constexpr bool kSets = false;
#endif
#ifdef RAYZ_TRACE_KERNEL_PRIMARY
    constexpr bool kPrimary = RAYZ_TRACE_KERNEL_PRIMARY; // camera segments from the pixels' primary lists
#else
    constexpr bool kPrimary = false;
#endif
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    PathState<R> p[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) path_init<R>(p[r]);
    uint32_t nseg = 0;
    WaveQueue wq; // wave-uniform
#ifdef RAYZ_FLAT_PROFILE // measurement build only: wave time per phase (refill, ray setup, scan, narrow flush, shade)
    unsigned long long ft[5] = {0, 0, 0, 0, 0}, ft0 = __builtin_amdgcn_s_memtime(), fiters = 0;
#define RAYZ_FPROF(k) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); ft[k] += now_ - ft0; ft0 = now_; }
#else
#define RAYZ_FPROF(k)
#endif

    for (;;) {
        // ---- retire finished chunks, refill idle slots ----
        bool any = false;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            path_refill<R, kAdaptive>(p[r], A, lane, wq);
            any = any || p[r].alive;
        }
        if (__ballot(any) == 0ull) break; // queue drained and every slot idle: the wave is done

        RAYZ_FPROF(0)
        // ---- nearest hit (full EXEC; idle tail slots recompute their last ray, results unused) ----
        ScanRay<R, kBasis> ray[NR];
        V<R> ud[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            ud[r] = unit(p[r].d);
            scan_begin<R, NR>(ray[r], p[r].o, p[r].d, ud[r], p[r].time);
        }
        RAYZ_FPROF(1)
        // ---- list phase (kPrimary): fresh paths on pixels with a list; the scan waits until the wave has none ----
        bool listed[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) listed[r] = false;
        bool list_phase = false;
        if constexpr (kPrimary) {
            uint32_t lp[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                lp[r] = 0u;
                if (p[r].alive && p[r].seg == 0u) {
                    lp[r] = p[r].item - (p[r].item / A.shard_pixels) * A.shard_pixels; // the local pixel (place_item, rows as they come)
                    listed[r] = A.primary[lp[r]] != rayz_primary::kNoList;
                }
                list_phase = list_phase || listed[r];
            }
            list_phase = __ballot(list_phase) != 0ull;
            if (list_phase) {
#pragma unroll
                for (int r = 0; r < NR; ++r)
                    if (listed[r]) { // scan_begin's tbest, ibest and inv_a2; every listed slot decided by the narrow phase
                        const uint32_t count = A.primary[lp[r]];
                        for (uint32_t j = 0; j < count; ++j) {
                            const uint32_t slot = A.primary[(size_t)(j + 1u) * A.shard_pixels + lp[r]];
                            narrow_eval<R>(A.sc.slot64[2 * slot], A.sc.slot64[2 * slot + 1], (int)A.sc.slot_pool[slot], ray[r].o, ray[r].d,
                                           ray[r].time, ray[r].inv_a2, A.tmin, ray[r].tbest, ray[r].ibest);
                        }
                    }
                RAYZ_FPROF(0) // (measurement builds: the list phases count as refill)
            }
        }
        if (!list_phase) {
#ifdef RAYZ_FLAT_PROFILE
            fiters++;
            scan_sphere_classes<R, NR, kSets>(A.sc, ray, A.tmin);
            RAYZ_FPROF(2)
            narrow_flush<R, NR>(A.sc, ray, A.tmin);
            scan_triangles<R, NR>(A.sc, ray, A.tmin);
            RAYZ_FPROF(3)
#else
            scan_spheres<R, NR, kSets>(A.sc, ray, A.tmin);
#endif
        }

        // ---- shade ----
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (p[r].alive && (!list_phase || listed[r])) {
                nseg++;
                p[r].seg++;
                bool cont = shade<R>(A.sc, p[r].g, p[r].o, p[r].d, ud[r], p[r].time, ray[r].tbest, ray[r].ibest, p[r].thr,
                                     p[r].acc);
                if (p[r].seg >= A.max_bounces) cont = false; // depth exhausted → black, src/renderer.zig:104-105
                p[r].alive = cont;
            }
        RAYZ_FPROF(4)
    }
#ifdef RAYZ_FLAT_PROFILE
    if (lane == 0) {
        for (int k = 0; k < 5; ++k) atomicAdd(&A.counters[4 + k], ft[k]);
        atomicAdd(&A.counters[9], fiters);
    }
#endif
    // ---- counters: one atomic per wave ----
    unsigned long long tot = nseg;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off);
    if (lane == 0) atomicAdd(&A.counters[1], tot);
}
