// experiments/launch.hpp — RETIRED: the host side of the two experiment kernels (bvh2_kernel.hpp, bvhx_kernel.hpp): how they are
// launched, what their measurement builds report and which debug knobs they take.  Included by rayz_hip.hip inside its anonymous
// namespace, in front of trace_window, and only under -DRAYZ_EXPERIMENTS; the product build has empty hooks of the same names there.
#pragma once

// BvhLaunchPlan::experiment: which kernel ran = its RAYZ_DEBUG_BVH_KERNEL value (0: a product kernel)
constexpr int kExperimentTwoPaths = 2; // trace_kernel_bvh2 (f32 only: same image, 19 % slower)
constexpr int kExperimentExchange = 3; // trace_kernel_bvhx (f32 only: round 4's walker / shader waves)

// Called with the product's plan of a BVH launch: swaps in the kernel RAYZ_DEBUG_BVH_KERNEL asks for, with its workgroup, its
// stacks, its share of LDS and its scheduling thresholds.
template <class R>
int experiment_override(BvhLaunchPlan<R>& plan, TraceArgs<R>& A, const RayzScene* s, const SceneBuffers<R>& b, const RayzRenderParams* p) {
    if constexpr (sizeof(R) == 4) {
        const long long which = tuning(RAYZ_DEBUG_BVH_KERNEL, 1);
        if (which == kExperimentTwoPaths) {
            plan.experiment = kExperimentTwoPaths;
            plan.kernel = b.quantized ? trace_kernel_bvh2<float, true> : trace_kernel_bvh2<float, false>;
            plan.block = (int)kBvh2Wg;
            plan.items_per_lane = 2; // (a lane of the two-path kernel holds two items)
            plan.stack_bytes = bvh_stack_bytes(s->bvh_dev.depth, kBvh2Wg);
            // three 256-thread workgroups per CU: less LDS to spare, a prefix of the top
            plan.top_records = std::min<uint32_t>(plan.top_records, b.quantized ? 512u : 256u);
            A.bvh_keep = (uint32_t)tuning(RAYZ_DEBUG_BVH2_KEEP, kBvh2Service | (kBvh2Blocked << 8) | (kBvh2Swap << 16) | (kBvhKeepStepping << 24));
        } else if (which == kExperimentExchange) {
            plan.experiment = kExperimentExchange;
            plan.kernel = b.quantized ? trace_kernel_bvhx<true> : trace_kernel_bvhx<false>;
            const long long xk = tuning(RAYZ_DEBUG_BVHX, -1);
            const uint32_t ns = xk < 0 ? 24u : (uint32_t)(xk & 0xff), xmin = xk < 0 ? 12u : (uint32_t)((xk >> 8) & 0xff),
                           xbatch = xk < 0 ? 48u : (uint32_t)((xk >> 16) & 0xff), xpat = xk < 0 ? 8u : (uint32_t)((xk >> 24) & 0xff),
                           xprio = xk < 0 ? 0x6eu : (uint32_t)((xk >> 32) & 0xff); // shader | walker box steps << 2 | leaf / root phases << 4 | exchange << 6
            A.x_slots = ns;
            A.x_cfg = xmin | (xbatch << 8) | (xpat << 16) | (xprio << 24);
            plan.stack_bytes = bvh_stack_bytes(s->bvh_dev.depth, kXWalkerLanes); // only its walker waves have stacks
            plan.extra_lds_bytes = bvhx_exchange_bytes(ns); // the slot area, after the oversized hittables' records
            if (p->max_bounces >= (1u << 30)) return fail(RAYZ_ERR_BAD_ARG, "the exchange kernel packs flags into the segment count: max_bounces < 2^30");
            // the top: what the walkers' stacks and the slots leave of the budget
            const size_t fixed = plan.stack_bytes + (b.n_big_leaves ? kBvhBigLdsBytes : 0) + plan.extra_lds_bytes;
            const size_t room = fixed < kBvhLdsBudget ? kBvhLdsBudget - fixed : 0;
            plan.top_records = std::min<uint32_t>(plan.top_records, (uint32_t)(room / (b.quantized ? 32 : 64)));
            const long long cap = tuning(RAYZ_DEBUG_BVH_TOP, -1);
            if (cap >= 0) plan.top_records = std::min<uint32_t>(plan.top_records, (uint32_t)cap);
        }
    }
    return RAYZ_OK;
}

// Called once the launch knows its LDS layout: the exchange area starts `words` u32s in, behind the oversized hittables' records.
template <class R> void experiment_lds_placed(TraceArgs<R>& A, uint32_t words) { A.x_words = words; }

// scene_sync after a render with a retired kernel (`c`: the render's 32 counters): the phase profile of a -DRAYZ_BVH_PROFILE
// build, then the exchange kernel's abort flag.
inline int experiment_sync(int experiment, const unsigned long long* c) {
#ifdef RAYZ_BVH_PROFILE
    if (experiment == kExperimentExchange) {
        const double wt = (double)(c[4] + c[5] + c[6]), stt = (double)(c[12] + c[13] + c[14]);
        std::fprintf(stderr, "bvhx walkers (share of wave time): exchange %.1f%% | idle (nobody walks) %.1f%% | rounds %.1f%%; per exchange: %.0f ticks; "
                             "at the start of a run of rounds: %.1f lanes walking, %.1f lanes hold a path; runs of rounds %.3g, exchanges %.3g\n",
                     100.0 * c[4] / wt, 100.0 * c[5] / wt, 100.0 * c[6] / wt, (double)c[4] / (double)(c[7] ? c[7] : 1), (double)c[8] / (double)(c[10] ? c[10] : 1),
                     (double)c[9] / (double)(c[10] ? c[10] : 1), (double)c[10], (double)c[7]);
        std::fprintf(stderr, "bvhx shaders (share of wave time): idle, nothing finished %.1f%% | waiting for a batch %.1f%% | pass %.1f%% (%.0f ticks per pass); "
                             "%.1f paths per pass, %.1f finished slots seen; passes %.3g\n",
                     100.0 * c[12] / stt, 100.0 * c[13] / stt, 100.0 * c[14] / stt, (double)c[14] / (double)(c[15] ? c[15] : 1),
                     (double)c[16] / (double)(c[15] ? c[15] : 1), (double)c[17] / (double)(c[15] ? c[15] : 1), (double)c[15]);
    } else if (experiment == kExperimentTwoPaths) {
        const double tot = (double)(c[4] + c[5] + c[6] + c[7] + c[8]);
        auto per = [&](int k) { return (double)c[9 + k] / (double)(c[10 + k] ? c[10 + k] : 1); };
        std::fprintf(stderr,
                     "bvh2 phases (share of wave time | mean lanes): service %.1f%% %.1f | swap %.1f%% %.1f | N %.1f%% %.1f | L %.1f%% %.1f | "
                     "C %.1f%% %.1f\n",
                     100.0 * c[4] / tot, per(0), 100.0 * c[5] / tot, per(2), 100.0 * c[6] / tot, per(4), 100.0 * c[7] / tot, per(6),
                     100.0 * c[8] / tot, per(8));
        const double it = (double)(c[14] ? c[14] : 1);
        std::fprintf(stderr, "  box steps: lanes per wave-step — stepping %.1f | parked at a leaf %.1f | walker idle %.1f; wave-steps per segment "
                             "%.2f; service passes %.3g, swaps %.3g, leaf phases %.3g\n",
                     per(4), (double)c[19] / it, (double)c[20] / it, it / (double)(c[1] ? c[1] : 1), (double)c[10], (double)c[12], (double)c[16]);
    }
#else
    (void)experiment;
#endif
    if (c[31] == 2)
        return fail(RAYZ_ERR_STATE, "the exchange kernel gave up waiting for a hand-over between its waves (bounded wait, no result)");
    return RAYZ_OK;
}

// rayz_hip_debug_set's check of the retired kernels' knobs (value ≥ 0): values their loop control cannot take are refused.
inline int experiment_knob_check(uint32_t knob, long long value) {
    auto lane_count = [](long long b) { return b >= 1 && b <= 64; }; // a threshold counted in lanes of a wave
    switch (knob) {
    case RAYZ_DEBUG_BVH_KERNEL:
        if (value < 1 || value > 3) return fail(RAYZ_ERR_BAD_ARG, "BVH_KERNEL %lld: 1, 2 or 3", value);
        break;
    case RAYZ_DEBUG_BVH2_KEEP: // service | blocked << 8 | swap << 16 | keep_stepping << 24
        if (value >> 32 || !lane_count(value & 0xff) || !lane_count((value >> 8) & 0xff) || !lane_count((value >> 16) & 0xff) ||
            !lane_count((value >> 24) & 0xff))
            return fail(RAYZ_ERR_BAD_ARG, "BVH2_KEEP 0x%llx: every threshold must be 1 .. 64 lanes", (unsigned long long)value);
        break;
    case RAYZ_DEBUG_BVHX: { // slots | exchange threshold << 8 | minimum batch << 16 | patience << 24 | priority << 32
        const long long ns = value & 0xff;
        if (value >> 40 || ns < 4 || ns > 64 || (ns & 1) || !lane_count((value >> 8) & 0xff) || !lane_count((value >> 16) & 0xff))
            return fail(RAYZ_ERR_BAD_ARG, "BVHX 0x%llx: slots even 4 .. 64, thresholds 1 .. 64 lanes", (unsigned long long)value);
        break;
    }
    default: break;
    }
    return RAYZ_OK;
}
