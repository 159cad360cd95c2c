// trace_kernel_bvh.hpp — the text of the one-path BVH trace kernel.  trace_kernels_bvh.hpp includes it once per kernel, lists the
// kernels and describes the round; see trace_kernel_flat.hpp for why one text and not one function.  No include guard.  An includer
// defines RAYZ_TRACE_KERNEL_NAME (required) and, for an adaptive pass's kernel, RAYZ_TRACE_KERNEL_ADAPTIVE true
// (default false); the text undefines both at its end.
#ifndef RAYZ_TRACE_KERNEL_NAME
#error "define RAYZ_TRACE_KERNEL_NAME before including trace_kernel_bvh.hpp"
#endif
#ifndef RAYZ_TRACE_KERNEL_ADAPTIVE
#define RAYZ_TRACE_KERNEL_ADAPTIVE false
#endif
template <class R, bool QUANT> __global__ __launch_bounds__(RAYZ_BVH_WG, (bvh_waves<R>() * 256 >= RAYZ_BVH_WG ? bvh_waves<R>() * 256 / RAYZ_BVH_WG : 1))
void RAYZ_TRACE_KERNEL_NAME(const TraceArgs<R> A) {
    constexpr bool kAdaptive = RAYZ_TRACE_KERNEL_ADAPTIVE; // work items over the active list (place_item)
    typedef typename VecOf<R>::type r4;
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const uint32_t n_nodes = A.sc.bvh_n_nodes;
    const int keep_active = (int)(A.bvh_keep & 0xffu), keep_stepping = (int)((A.bvh_keep >> 8) & 0xffu);
    const float tmin32 = round_down_f32(A.tmin); // the box steps' tmin
    Pcg32 g{0, 1};
    V<R> o{0, 0, 0}, d{0, 0, 1}, ud{0, 0, 1}, thr{1, 1, 1}, acc{0, 0, 0};
    BvhQuery<R> q;
    q.qa = {1.0f, 1.0f, 1.0f};
    q.qb = {0.0f, 0.0f, 0.0f};
    q.tb32 = 0.0f;
    q.inv_a2 = 1.0;
    q.tbest = R(0);
    q.ibest = -1;
    q.cur = kBvhDone;
    q.sp = 0;
    q.top = kBvhDone;
    q.lb.make(ud, o);
    // dynamic shared memory, from LDS address 0 (the kernel has no static LDS): the top of the tree, copied once per
    // workgroup (A.bvh_top_words u32s; a node's LDS address is its index << 6 for f32), then the per-lane traversal stacks,
    // sized by the launch from the tree's depth: entry s of this lane at stack[256 * s] — conflict-free for any mix of s
    extern __shared__ uint32_t lds_words[];
    // the node fetch addresses the LDS copy by index << 6 from LDS address 0: refuse to run (loudly: the host turns the
    // flag into RAYZ_ERR_STATE) should a build ever place anything in front of the dynamic segment
    if ((uint32_t)(uintptr_t)(__attribute__((address_space(3))) uint32_t*)lds_words != 0u) {
        if (threadIdx.x == 0) A.counters[31] = 1ull;
        return;
    }
    f4* top = (f4*)lds_words;
    uint32_t* stack = lds_words + A.bvh_top_words + kBvhWg + threadIdx.x; // (one guard row under entry 0: BvhQuery::top)
    for (uint32_t k = threadIdx.x; k < A.sc.bvh_top / 16u; k += kBvhWg) top[k] = A.sc.bvh_nodes[k];
    const f4* nodes_base = scalar_base(A.sc.bvh_nodes);
    stack[0] = kBvhDone; // the sentinel under every lane's stack
    // the oversized hittables' records, entry e = 2·(descriptor) + (entry of it): {filter record: 3 words in R, f64 sphere: 2}
    unsigned char* big_lds = (unsigned char*)(lds_words + A.bvh_big_words);
    if (threadIdx.x < 2u * A.sc.bvh_n_big_leaves) {
        const uint32_t desc = A.sc.bvh_big[threadIdx.x >> 1], j = threadIdx.x & 1u;
        if (j < (desc & 3u)) {
            const uint32_t slot = (desc >> 4) + j;
            d4* dst64 = (d4*)(big_lds + threadIdx.x * bvh_big_entry_bytes<R>());
            dst64[0] = A.sc.bvh_sph64[2 * slot];
            dst64[1] = A.sc.bvh_sph64[2 * slot + 1];
            r4* dst = (r4*)(dst64 + 2);
            const r4* rec = A.sc.bvh_leaf + (size_t)A.sc.bvh_leaf_stride * slot;
            dst[0] = rec[0];
            dst[1] = rec[1];
            dst[2] = A.sc.bvh_leaf_stride > 2u ? rec[2] : rec[1];
        }
    }
    __syncthreads();
    R time = 0;
    uint32_t item = 0, px = 0, py = 0, s_cur = 0, s_end = 0, seg = 0, nseg = 0, sphere_tests = 0;
    uint32_t node_tests = 0; // counted per WAVE (two per stepping lane, off the step's own lane count): scalar arithmetic
    bool has_item = false, alive = false, fresh = false;
    WaveQueue wq; // wave-uniform
#ifdef RAYZ_BVH_PROFILE
    unsigned long long pt[5] = {0, 0, 0, 0, 0}, pl[7] = {0, 0, 0, 0, 0, 0, 0}, px3[3] = {0, 0, 0}, pt0 = __builtin_amdgcn_s_memtime(), fetch_ticks = 0;
#define RAYZ_PROF_T(k) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); pt[k] += now_ - pt0; pt0 = now_; }
#define RAYZ_PROF_L(k, n) { pl[k] += (unsigned long long)(n); pl[k + 1] += 1; }
#else
#define RAYZ_PROF_T(k)
#define RAYZ_PROF_L(k, n)
#endif

    for (;;) {
        // ---- retire finished chunks, refill idle lanes (wave-aggregated queue pop) ----
        if (!alive && has_item && s_cur == s_end) {
            A.partial[item] = r4{acc.x, acc.y, acc.z, R(0)};
            has_item = false;
        }
        {
            const bool popping = __ballot(!alive && !has_item && !queue_empty<R>(wq, A)) != 0ull;
            uint32_t got_item = 0;
            if (queue_pop<R>(A, wq, lane, !alive && !has_item && !queue_empty<R>(wq, A), got_item)) {
                item = got_item;
                has_item = true;
                const uint32_t k = place_item<R, true, kAdaptive>(A, item, px, py);
                chunk_bounds<R>(A, k, s_cur, s_end);
                acc = {R(0), R(0), R(0)};
            }
            // the per-lane u32 statistics would wrap after ≈30 minutes inside one launch: spill them when half full
            if (popping && node_tests > RAYZ_STAT_SPILL) {
                if (lane == 0) atomicAdd(&A.counters[2], (unsigned long long)node_tests);
                atomicAdd(&A.counters[3], (unsigned long long)sphere_tests);
                atomicAdd(&A.counters[1], (unsigned long long)nseg);
                node_tests = sphere_tests = nseg = 0;
            }
        }
        if (!alive && has_item) {
            const unsigned long long pixel_index = (unsigned long long)py * A.width + px;
            g.seed_path(A.seed, pixel_index * A.spp + s_cur);
            camera_ray<R>(A.cam, g, px, py, o, d, time);
            thr = {R(1), R(1), R(1)};
            seg = 0;
            s_cur++;
            alive = true;
            fresh = true;
        }
        if (__ballot(alive) == 0ull) break;
        // ---- every segment that starts here (camera rays above, scattered rays of the last shading pass): one place
        //      for the per-segment set-up (unit direction, slab constants) ----
        if (fresh) {
            ud = unit(d);
            bvh_begin<R, QUANT>(q, A.sc, o, d, ud, n_nodes);
        }
        // .. then the oversized hittables kept out of the tree: the walk starts with their tbest and culls behind it
        if (A.sc.bvh_n_big_leaves != 0u && __ballot(fresh) != 0ull) {
            if (fresh) {
                for (uint32_t k = 0; k < A.sc.bvh_n_big_leaves; ++k) { // wave-uniform trip count
                    const uint32_t desc = A.sc.bvh_big[k];
                    sphere_tests += desc & 3u;
                    for (uint32_t j = 0; j < (desc & 3u); ++j) { // (from the LDS copy: the same address in every lane)
                        const d4* rec64 = (const d4*)(big_lds + (2u * k + j) * bvh_big_entry_bytes<R>());
                        const r4* rec = (const r4*)(rec64 + 2);
                        const r4 c = rec[0], v = rec[1], w = rec[2];
                        if (bvh_leaf_eval<R>(A.sc, q, desc, j, c, v, o, d, ud, time, A.tmin, &w) != 0u)
                            bvh_candidate_eval<R>(q, rec64[0], rec64[1], (int)bits(v.w), o, d, time, A.tmin);
                    }
                }
            }
        }
        fresh = false;
        RAYZ_PROF_T(0)

        // ---- rounds of (N) box steps, (L) leaf tests, (C) candidate roots ----
        const int n_alive = __popcll(__ballot(alive));
        for (;;) {
            if constexpr (sizeof(R) == 8) q.tb32 = round_up_f32(q.tbest); // (tbest moves in phases L and C and in the set-up
                                                                          //  above, never in N)
            // phase N: lanes holding an inner node step; lanes holding a leaf wait.  It goes on while at least keep_stepping
            // lanes can step — or any, if nobody waits at a leaf (ONE wave-uniform flag, computed where the lane count is
            // known: the loop has a single exit test)
            bool can_step = q.cur < kBvhDone;
            int n_can = __popcll(__ballot(can_step));
            // (n_can != 0 first: with nobody able to step the loop must end whatever the threshold is — a threshold of 0 would
            //  otherwise spin for ever with no lane stepping)
            bool run = n_can != 0 && (n_can >= keep_stepping || __ballot((int32_t)q.cur < 0) == 0ull);
            // (wave priorities: the rounds' dependent chains — box steps above leaf and root phases — ahead of the throughput
            //  work of the shading pass and the refill, which other waves' issue slots serve as well late as early:
            //  +0.9 % config 3, +1.7 % config 5, profiles/r03/bvh_step/setprio.log)
            __builtin_amdgcn_s_setprio(3);
            while (run) {
                RAYZ_PROF_L(0, n_can)
#ifdef RAYZ_BVH_PROFILE
                px3[0] += __popcll(__ballot((int32_t)q.cur < 0));
                px3[1] += __popcll(__ballot(alive && q.cur == kBvhDone));
                px3[2] += __popcll(__ballot(!alive));
                if (can_step) bvh_node_step<R, kBvhWg, QUANT>(A.sc, nodes_base, q, tmin32, stack, fetch_ticks);
#else
                if (can_step) bvh_node_step<R, kBvhWg, QUANT>(A.sc, nodes_base, q, tmin32, stack);
                // .. and a second step for the lanes that still hold an inner node, without a new wave-level decision (lane
                // counts against thresholds are scalar work with a taken branch at its end: every other step is enough —
                // +1 % on configs 3 / 5, +2.6 % on config 2, profiles/r03/bvh_step/unroll.log; three or four lose it again)
                {
                    const bool again = q.cur < kBvhDone;
                    node_tests += 2u * (uint32_t)__popcll(__ballot(again));
                    if (again) bvh_node_step<R, kBvhWg, QUANT>(A.sc, nodes_base, q, tmin32, stack);
                }
#endif
                node_tests += 2u * (uint32_t)n_can;
                can_step = q.cur < kBvhDone;
                n_can = __popcll(__ballot(can_step));
                run = n_can != 0 && (n_can >= keep_stepping || __ballot((int32_t)q.cur < 0) == 0ull);
            }
            __builtin_amdgcn_s_setprio(2);
            RAYZ_PROF_T(1)
            const bool parked = (int32_t)q.cur < 0;
            if (__ballot(parked) == 0ull) break; // nobody parked: every walking lane ran out of nodes
            RAYZ_PROF_L(2, __popcll(__ballot(parked)))
            uint32_t cand0 = 0, cand1 = 0;
            int pool0 = 0, pool1 = 0;
            if (parked) { // phase L
                const uint32_t leaf = q.cur & ~kBvhLeafFlag;
                sphere_tests += leaf & 3u;
                bvh_pop<R, kBvhWg>(q, stack); // first: its LDS read-ahead travels while the records are fetched and tested
                bvh_leaf_pair<R>(A.sc, q, leaf, o, d, ud, time, A.tmin, cand0, cand1, pool0, pool1);
            }
            RAYZ_PROF_T(2)
            if (__ballot((cand0 | cand1) != 0u) != 0ull) { // phase C (bvh_candidate_passes, restated)
                RAYZ_PROF_L(4, __popcll(__ballot((cand0 | cand1) != 0u)))
                // a lane's only candidate goes into the first pass whichever entry it came from: the second pass runs
                // only when some lane has two (the nearest hit does not depend on the order)
                const uint32_t c0 = cand0 != 0u ? cand0 : cand1, c1 = cand0 != 0u ? cand1 : 0u;
                const int p0 = cand0 != 0u ? pool0 : pool1;
                if (c0 != 0u) bvh_candidate<R>(A.sc, q, c0 - 1u, p0, o, d, time, A.tmin);
                if (__ballot(c1 != 0u) != 0ull) {
                    if (c1 != 0u) bvh_candidate<R>(A.sc, q, c1 - 1u, pool1, o, d, time, A.tmin);
                }
            }
            RAYZ_PROF_T(3)
            const int n_walking = __popcll(__ballot(q.cur != kBvhDone));
            if (n_walking == 0) break;
            if (n_walking < keep_active && n_walking < n_alive) break; // finished lanes wait: go shade / refill them
        }
        __builtin_amdgcn_s_setprio(0);

        // ---- shade lanes whose query is complete ----
        RAYZ_PROF_T(1)
#ifdef RAYZ_BVH_PROFILE
        pl[6] += __ballot(alive && q.cur == kBvhDone) != 0ull ? 1ull : 0ull; // shade passes
#endif
        if (alive && q.cur == kBvhDone) {
            nseg++;
            seg++;
            bool cont = shade<R>(A.sc, g, o, d, ud, time, q.tbest, q.ibest, thr, acc);
            if (seg >= A.max_bounces) cont = false;
            alive = cont;
            fresh = cont;
            // until its set-up runs at the top of the loop the lane must not look finished: no node, empty stack, but
            // `fresh` keeps it out of the next shading pass (the set-up always comes first)
        }
        RAYZ_PROF_T(4)
    }
#ifdef RAYZ_BVH_PROFILE
    RAYZ_PROF_T(4)
    if (lane == 0) {
        for (int k = 0; k < 5; ++k) atomicAdd(&A.counters[4 + k], pt[k]);
        for (int k = 0; k < 7; ++k) atomicAdd(&A.counters[9 + k], pl[k]);
        for (int k = 0; k < 3; ++k) atomicAdd(&A.counters[16 + k], px3[k]);
        atomicAdd(&A.counters[19], fetch_ticks);
    }
#endif
    unsigned long long t0 = nseg, t1 = node_tests, t2 = sphere_tests;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        t0 += __shfl_xor(t0, off);
        t2 += __shfl_xor(t2, off);
    }
    if (lane == 0) {
        atomicAdd(&A.counters[1], t0);
        atomicAdd(&A.counters[2], t1);
        atomicAdd(&A.counters[3], t2);
    }
}
#undef RAYZ_TRACE_KERNEL_NAME
#undef RAYZ_TRACE_KERNEL_ADAPTIVE
