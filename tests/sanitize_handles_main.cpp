// The frame-filter handles' host code (rayz_amd/csrc/frame_handle.hpp, denoiser.hpp, temporal.hpp) under AddressSanitizer and
// UndefinedBehaviorSanitizer, on the CPU: the whole host library is compiled in (host side only), no device is ever initialised.
// Every refusal of the denoiser's and the temporal handle's entry points is walked with its message checked, in the documented
// order (every argument before the handle); then handles built here by hand — what create leaves, minus the device memory — go
// through the handle checks, the stream resolution, the timing refusals and destroy.  tests/test_sanitizers.py builds and runs it.
#include "../rayz_amd/csrc/rayz_hip.hip"

#include <cstdio>
#include <cstring>

static int bad = 0;

static void expect(int rc, int want, const char* text, const char* what) {
    const char* msg = rayz_hip_last_error();
    if (rc != want || (text && !std::strstr(msg, text))) {
        std::printf("FAIL %s: rc %d (want %d), message \"%s\" (want \"%s\")\n", what, rc, want, msg, text ? text : "");
        ++bad;
    }
}

template <class H> static H* by_hand(uint32_t w, uint32_t h) { // a handle as create leaves it, without buffers or events
    H* x = new H;
    x->magic = H::kMagic, x->device = 0, x->width = w, x->height = h;
    return x;
}

int main() {
    float buf[4] = {};
    int32_t idx[4] = {};
    RayzQueryOutputs g{};
    g.index = idx, g.normal = buf, g.point = buf, g.albedo = buf;

    // ---- create: both nouns, no device -------------------------------------------------------------------------------------------
    RayzDenoiser* dn = (RayzDenoiser*)buf;
    RayzTemporal* tm = (RayzTemporal*)buf;
    expect(rayz_hip_denoiser_create(-1, 4, 4, nullptr), RAYZ_ERR_BAD_ARG, "out handle pointer is null", "denoiser create, null out");
    expect(rayz_hip_denoiser_create(-1, 0, 4, &dn), RAYZ_ERR_BAD_ARG, "denoiser frame 0x4: zero size", "denoiser create, zero size");
    if (dn) ++bad, std::printf("FAIL: a refused create left a handle\n");
    expect(rayz_hip_denoiser_create(-1, 65536, 65536, &dn), RAYZ_ERR_BAD_ARG, "denoiser frame 65536x65536: more than RAYZ_DENOISE_MAX_PIXELS pixels",
           "denoiser create, too large");
    expect(rayz_hip_denoiser_create(-1, 4, 4, &dn), RAYZ_ERR_NO_DEVICE, "rayz_hip_init has not succeeded", "denoiser create, no default device");
    expect(rayz_hip_temporal_create(-1, 4, 4, nullptr), RAYZ_ERR_BAD_ARG, "out handle pointer is null", "temporal create, null out");
    expect(rayz_hip_temporal_create(-1, 4, 0, &tm), RAYZ_ERR_BAD_ARG, "temporal frame 4x0: zero size", "temporal create, zero size");
    expect(rayz_hip_temporal_create(-1, 65536, 65536, &tm), RAYZ_ERR_BAD_ARG, "temporal frame 65536x65536: more than RAYZ_DENOISE_MAX_PIXELS pixels",
           "temporal create, too large");
    expect(rayz_hip_temporal_create(-1, 4, 4, &tm), RAYZ_ERR_NO_DEVICE, "rayz_hip_init has not succeeded", "temporal create, no default device");
    if (tm) ++bad, std::printf("FAIL: a refused create left a handle\n");

    // ---- the denoiser's runs: every argument before the handle (which is null throughout) -------------------------------------------
    RayzDenoiseGuidedParams gp{0, 6, RAYZ_DENOISE_ALBEDO, 0, 2.0, 0.25, 1e-4};
    RayzDenoiseParams pp{0, 6, RAYZ_DENOISE_ALBEDO, 0, 0.5, 0.25};
    auto plain = [&](const RayzDenoiseParams& p, const float* in, const RayzQueryOutputs* gb, float* out) {
        return rayz_hip_denoiser_run(nullptr, &p, in, gb, out, nullptr);
    };
    auto guided = [&](const RayzDenoiseGuidedParams& p, const float* in, const float* var, const RayzQueryOutputs* gb, float* out) {
        return rayz_hip_denoiser_run_guided(nullptr, &p, in, var, gb, out, nullptr, nullptr);
    };
    for (int mode = 0; mode < 2; ++mode) {
        auto run = [&](RayzDenoiseGuidedParams p, const float* in = nullptr, const RayzQueryOutputs* gb = nullptr, float* out = nullptr,
                       const float* var = nullptr) {
            if (mode) return guided(p, in, var, gb, out);
            return plain(RayzDenoiseParams{p.levels, p.normal_power_log2, p.flags, 0, p.sigma_color, p.sigma_plane}, in, gb, out);
        };
        const char* m = mode ? "guided" : "plain";
        auto p = gp;
        p.levels = 9;
        expect(run(p), RAYZ_ERR_BAD_ARG, "denoise levels 9 > 8", m);
        p = gp, p.normal_power_log2 = 17;
        expect(run(p), RAYZ_ERR_BAD_ARG, "denoise normal_power_log2 17 > 16", m);
        p = gp, p.flags = 6;
        expect(run(p), RAYZ_ERR_BAD_ARG, "unknown denoise flag bits 0x6", m);
        p = gp, p.sigma_color = 0;
        expect(run(p), RAYZ_ERR_BAD_ARG, "denoise sigma_color 0: must be positive", m);
        p = gp, p.sigma_plane = 1e-30;
        expect(run(p), RAYZ_ERR_BAD_ARG, "denoise sigma_plane 1e-30: must be positive (and its square in f32)", m);
        p = gp, p.var_floor = 0;
        if (mode) expect(run(p), RAYZ_ERR_BAD_ARG, "denoise var_floor 0: must be positive", m);
        else expect(run(p), RAYZ_ERR_BAD_ARG, "denoise: null colour buffer", m); // (the plain mode has no var_floor)
        expect(run(gp, buf, &g, nullptr, buf), RAYZ_ERR_BAD_ARG, "denoise: null colour buffer", m);
        if (mode) expect(run(gp, buf, &g, buf, nullptr), RAYZ_ERR_BAD_ARG, "denoise: the guided mode needs the per-channel variance", m);
        expect(run(gp, buf, nullptr, buf, buf), RAYZ_ERR_BAD_ARG, "denoise: null G-buffer", m);
        RayzQueryOutputs h = g;
        h.point = nullptr;
        expect(run(gp, buf, &h, buf, buf), RAYZ_ERR_BAD_ARG, "denoise: the G-buffer needs index, normal and point", m);
        h = g, h.albedo = nullptr;
        expect(run(gp, buf, &h, buf, buf), RAYZ_ERR_BAD_ARG, "denoise: RAYZ_DENOISE_ALBEDO needs the G-buffer's albedo", m);
        p = gp, p.flags = 0;
        expect(run(p, buf, &h, buf, buf), RAYZ_ERR_STATE, "not a denoiser handle", m); // (without the flag the albedo is not asked for)
        expect(run(gp, buf, &g, buf, buf), RAYZ_ERR_STATE, "not a denoiser handle", m);
    }
    expect(rayz_hip_denoiser_run(nullptr, nullptr, buf, &g, buf, nullptr), RAYZ_ERR_STATE, "not a denoiser handle", "plain, default params");
    expect(rayz_hip_denoiser_run_guided(nullptr, nullptr, buf, buf, &g, buf, nullptr, nullptr), RAYZ_ERR_STATE, "not a denoiser handle",
           "guided, default params");
    (void)pp;

    // ---- the temporal step ------------------------------------------------------------------------------------------------------
    RayzCameraDesc cam{};
    cam.px_du[0] = 1, cam.px_dv[1] = 1, cam.px_origin[2] = 1;
    const RayzTemporalParams tp{0.05, 65536.0, 0.9, 0.05};
    auto step = [&](RayzTemporalParams p, const RayzCameraDesc* c, uint32_t spp, const float* in, const float* var, const RayzQueryOutputs* gb,
                    float* out, float* vout, RayzTemporal* h = nullptr) {
        return rayz_hip_temporal_step(h, &p, c, spp, in, var, gb, out, vout, nullptr, nullptr);
    };
    auto t = tp;
    t.alpha_min = 2;
    expect(step(t, &cam, 8, buf, buf, &g, buf, buf), RAYZ_ERR_BAD_ARG, "temporal alpha_min 2: must lie in [0, 1]", "temporal");
    t = tp, t.n_max = 0.5;
    expect(step(t, &cam, 8, buf, buf, &g, buf, buf), RAYZ_ERR_BAD_ARG, "temporal n_max 0.5: must be at least 1", "temporal");
    t = tp, t.normal_cos_min = -2;
    expect(step(t, &cam, 8, buf, buf, &g, buf, buf), RAYZ_ERR_BAD_ARG, "temporal normal_cos_min -2: must lie in [-1, 1]", "temporal");
    t = tp, t.max_rel_dist = 0;
    expect(step(t, &cam, 8, buf, buf, &g, buf, buf), RAYZ_ERR_BAD_ARG, "temporal max_rel_dist 0: must be positive", "temporal");
    expect(step(tp, &cam, 0, buf, buf, &g, buf, buf), RAYZ_ERR_BAD_ARG, "temporal spp 0: must lie in 1 .. 2^24", "temporal");
    expect(step(tp, &cam, 8, nullptr, buf, &g, buf, buf), RAYZ_ERR_BAD_ARG, "temporal: null colour buffer", "temporal");
    expect(step(tp, &cam, 8, buf, buf, &g, buf, nullptr), RAYZ_ERR_BAD_ARG, "temporal: null variance buffer", "temporal");
    expect(step(tp, &cam, 8, buf, buf, nullptr, buf, buf), RAYZ_ERR_BAD_ARG, "temporal: null G-buffer", "temporal");
    RayzQueryOutputs h = g;
    h.index = nullptr;
    expect(step(tp, &cam, 8, buf, buf, &h, buf, buf), RAYZ_ERR_BAD_ARG, "temporal: the G-buffer needs index, normal and point", "temporal");
    expect(step(tp, nullptr, 8, buf, buf, &g, buf, buf), RAYZ_ERR_BAD_ARG, "temporal: null camera", "temporal");
    RayzCameraDesc flat{};
    expect(step(tp, &flat, 8, buf, buf, &g, buf, buf), RAYZ_ERR_BAD_ARG, "span no volume", "temporal");
    expect(step(tp, &cam, 8, buf, buf, &g, buf, buf), RAYZ_ERR_STATE, "not a temporal handle", "temporal");
    expect(rayz_hip_temporal_reset(nullptr), RAYZ_ERR_STATE, "not a temporal handle", "temporal reset");
    expect(rayz_hip_temporal_timing(nullptr, buf), RAYZ_ERR_STATE, "not a temporal handle", "temporal timing");
    expect(rayz_hip_denoiser_timing(nullptr, nullptr, buf, 4), RAYZ_ERR_STATE, "not a denoiser handle", "denoiser timing");
    expect(rayz_hip_denoiser_destroy(nullptr), RAYZ_OK, nullptr, "denoiser destroy(NULL)");
    expect(rayz_hip_temporal_destroy(nullptr), RAYZ_OK, nullptr, "temporal destroy(NULL)");

    // ---- handles built by hand: the checks behind the arguments, without a device -------------------------------------------------
    dn = by_hand<RayzDenoiser>(2, 2);
    tm = by_hand<RayzTemporal>(2, 2);
    // each is refused where the other is expected (both are live allocations larger than the fields read)
    expect(rayz_hip_denoiser_timing((RayzDenoiser*)tm, nullptr, buf, 4), RAYZ_ERR_STATE, "not a denoiser handle", "a temporal handle as a denoiser");
    expect(rayz_hip_temporal_reset((RayzTemporal*)dn), RAYZ_ERR_STATE, "not a temporal handle", "a denoiser as a temporal handle");
    expect(rayz_hip_denoiser_destroy((RayzDenoiser*)tm), RAYZ_ERR_STATE, "not a denoiser handle", "destroy of the wrong kind");
    // no stream given and the handle's device not initialised: refused before anything touches a device
    expect(rayz_hip_denoiser_run(dn, nullptr, buf, &g, buf, nullptr), RAYZ_ERR_NO_DEVICE, "device 0 is not initialised", "run, no device");
    expect(rayz_hip_denoiser_run_guided(dn, nullptr, buf, buf, &g, buf, nullptr, nullptr), RAYZ_ERR_NO_DEVICE, "device 0 is not initialised",
           "guided run, no device");
    expect(step(tp, &cam, 8, buf, buf, &g, buf, buf, tm), RAYZ_ERR_NO_DEVICE, "device 0 is not initialised", "step, no device");
    expect(rayz_hip_denoiser_timing(dn, nullptr, buf, 4), RAYZ_ERR_STATE, "no denoiser run to time", "timing before a run");
    expect(rayz_hip_temporal_timing(tm, buf), RAYZ_ERR_STATE, "no temporal step to time", "timing before a step");
    expect(rayz_hip_temporal_reset(tm), RAYZ_OK, nullptr, "reset");
    if (dn->last_ev != -1 || tm->last_ev != -1 || dn->levels_run || tm->has_history) ++bad, std::printf("FAIL: a refused call changed its handle\n");
    expect(rayz_hip_denoiser_destroy(dn), RAYZ_OK, nullptr, "denoiser destroy"); // (no event recorded: nothing to wait for)
    expect(rayz_hip_temporal_destroy(tm), RAYZ_OK, nullptr, "temporal destroy");

    std::printf(bad ? "FAILED\n" : "sanitizer run ok\n");
    return bad ? 1 : 0;
}
