"""The à-trous denoiser without a GPU: hand-derived known answers on the CPU restatement
(tests/denoise_mirror.cpp, which the GPU tests hold the kernels to bit for bit), the C ABI's refusals, and the quality condition —
a denoised 4-spp frame of the oracle is nearer to its 256-spp frame than the noisy one."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref
import query_reference as qr
from rayz_amd import capi, tracer

INF = float("inf")
K = np.array([1, 4, 6, 4, 1], dtype=np.float64) / 16  # {1/16, 1/4, 3/8, 1/4, 1/16}


def flat_guides(h, w):
    """One plane facing the camera: every normal (0, 0, 1), points on the grid z = 0 — n_p.n_q = 1 exactly, pl = n_p.v = 0 exactly,
    so wn = 1 and wz = (1 - 0)^2 = 1: the geometry term is 1 for every pair of pixels."""
    index = np.zeros((h, w), np.int32)
    normal = np.zeros((h, w, 3), np.float32)
    normal[..., 2] = 1
    point = np.zeros((h, w, 3), np.float32)
    point[..., 0], point[..., 1] = np.meshgrid(np.arange(w), np.arange(h))
    return index, normal, point


def run(rgb, index, normal, point, albedo=None, **kw):
    kw.setdefault("flags", 0 if albedo is None else denoise_ref.ALBEDO)
    return denoise_ref.denoise(rgb, index, normal, point, albedo, **kw)


def test_impulse_response_is_the_b3_spline_kernel():
    """One level, uniform guides (g = 1), sigma_color = +inf (wc = 1 / (1 + x / inf) = 1 / (1 + 0) = 1): w = h = k[i]·k[j], and in the
    interior W = (sum k)^2 = 1 exactly (all partial sums are multiples of 1/256 below 2).  An impulse of 256 at the centre reaches
    pixel p through the one tap q = centre, i.e. (i, j) = centre - p: out(p) = 256·k[i]·k[j] / 1, exact integers 1..36."""
    h = w = 11
    index, normal, point = flat_guides(h, w)
    rgb = np.zeros((h, w, 3), np.float32)
    rgb[5, 5] = (256, 512, 128)
    out = run(rgb, index, normal, point, levels=1, sigma_color=INF)
    want = np.zeros((h, w), np.float64)
    want[3:8, 3:8] = 256 * np.outer(K, K)
    assert np.array_equal(out[..., 0], want.astype(np.float32))
    assert np.array_equal(out[..., 1], 2 * out[..., 0]) and np.array_equal(out[..., 2], out[..., 0] / 2)
    # stride 2 (level 1 alone cannot be asked for, so: two levels on an impulse is level 1 applied to k (x) k): the second level's taps
    # are 2 pixels apart, so the response is the convolution of k (x) k with k (x) k upsampled by 2 — separable, exact in f32 here
    out2 = run(rgb, index, normal, point, levels=2, sigma_color=INF)
    k2 = np.zeros(9)
    k2[::2] = K
    kk = np.convolve(K, k2)  # 13 taps: reaches 6 pixels, but the frame ends 5 from the centre, where W is renormalised: check the inside
    want2 = 256 * np.outer(kk, kk)[1:12, 1:12]
    assert np.array_equal(out2[4:7, 4:7, 0], want2[4:7, 4:7].astype(np.float32))  # pixels whose 25 level-1 taps are all in the frame


def test_impulse_at_a_corner_is_renormalised_over_the_nine_taps_in_the_frame():
    """Impulse of 1 at pixel (0, 0).  Output pixel p = (x, y), x, y in 0..2, sees it through tap (i, j) = (-x, -y).  The taps of p that
    lie in the frame are i in -x..2, j in -y..2, so W = A(x)·A(y) with A(0) = 3/8 + 1/4 + 1/16 = 11/16, A(1) = 15/16, A(2) = 1 — W and
    every partial sum are multiples of 1/256, exact.  out(p) = k[-x]·k[-y] / (A(x)·A(y)), ONE correctly rounded f32 divide of exact
    operands: the f64 quotient of the same operands rounds to f32 identically (53 >= 2·24 + 2 bits)."""
    h, w = 6, 7
    index, normal, point = flat_guides(h, w)
    rgb = np.zeros((h, w, 3), np.float32)
    rgb[0, 0] = 1
    out = run(rgb, index, normal, point, levels=1, sigma_color=INF)
    A = {0: 11 / 16, 1: 15 / 16, 2: 1.0}
    kc = {0: 3 / 8, 1: 1 / 4, 2: 1 / 16}
    for y in range(h):
        for x in range(w):
            want = np.float32(kc[x] * kc[y] / (A[x] * A[y])) if x <= 2 and y <= 2 else np.float32(0)
            assert out[y, x, 0] == want, (x, y, out[y, x, 0], want)
    assert out[0, 0, 0] == np.float32((9 / 64) / (121 / 256))  # 36/121: the corner keeps more of its own value than the interior's 9/64


@pytest.mark.parametrize("levels", range(1, 9))
def test_a_constant_image_is_a_fixed_point(levels):
    """Δe = 0 so wc = 1 / (1 + 0 / sc2) = 1; w = h·g.  With a colour of at most 8 significant bits every product w·c and every partial
    sum S is exact when g is 1 (h is a multiple of 2^-8 with at most 6 bits; W <= 1 is a multiple of 2^-8), so S = c·W exactly and
    S / W = c — also at the frame's edges, where W < 1.  With real guides g is not 1 and S carries roundings: then the result is c to
    within the accumulated error: a level's output is a convex combination of its inputs (every w >= 0) computed with 25 FMAs into S,
    24 adds into W and one divide, each rounding <= 2^-24 relative (all terms positive): (1 + 2^-24)^(50·L) - 1 over L levels."""
    h, w = 37, 53
    index, normal, point = flat_guides(h, w)
    c = np.array([0.75, 3.5, 0.00390625 * 77], np.float32)
    rgb = np.broadcast_to(c, (h, w, 3)).copy()
    out = run(rgb, index, normal, point, levels=levels, sigma_color=0.5)
    assert np.array_equal(out, rgb)
    rng = np.random.default_rng(levels)
    normal = rng.normal(size=(h, w, 3)) * 0.05 + (0, 0, 1)
    normal = (normal / np.linalg.norm(normal, axis=2, keepdims=True)).astype(np.float32)
    point = point + rng.normal(scale=0.01, size=(h, w, 3)).astype(np.float32)
    c = np.array([0.1, 0.7, 1.3], np.float32)
    rgb = np.broadcast_to(c, (h, w, 3)).copy()
    out = run(rgb, index, normal, point, levels=levels, sigma_color=0.5, sigma_plane=0.5)
    bound = (1 + 2.0 ** -24) ** (50 * levels) - 1
    assert (np.abs(out.astype(np.float64) - rgb) <= bound * rgb).all()


def test_orthogonal_normals_do_not_mix():
    """Left half: normal (1, 0, 0), colour A; right half: normal (0, 1, 0), colour B.  Across the border n_p.n_q = fma(0, 0, fma(0, 1,
    1·0)) = 0 exactly: wn = 0, w = 0, the tap adds 0 to W and fma(0, e_q, S) = S.  Within a half the points lie in the half's own
    tangent plane (pl = 0 exactly: the coordinate along the normal is constant), wn = 1, wz = 1, g = 1, and the colour is constant, so
    each half is the constant-image case: unchanged bit for bit, for 8-bit colours.  (sigma_color = +inf: nothing but the normal
    keeps the halves apart.)"""
    h, w = 24, 40
    index = np.zeros((h, w), np.int32)
    normal = np.zeros((h, w, 3), np.float32)
    normal[:, :20, 0] = 1
    normal[:, 20:, 1] = 1
    point = np.zeros((h, w, 3), np.float32)
    gx, gy = np.meshgrid(np.arange(w), np.arange(h))
    point[:, :20, 1], point[:, :20, 2] = gx[:, :20], gy[:, :20]   # x = 0: the plane orthogonal to (1, 0, 0)
    point[:, 20:, 0], point[:, 20:, 2] = gx[:, 20:], gy[:, 20:]   # y = 0: the plane orthogonal to (0, 1, 0)
    rgb = np.zeros((h, w, 3), np.float32)
    rgb[:, :20] = (0.25, 0.5, 0.75)
    rgb[:, 20:] = (3, 0.125, 40)
    for levels in (1, 3, 5):
        out = run(rgb, index, normal, point, levels=levels, sigma_color=INF, sigma_plane=0.25)
        assert np.array_equal(out, rgb), levels


def test_background_and_hits_never_mix():
    """bg(p) != bg(q): the tap is skipped.  A hit region of constant colour A inside a background of constant colour B (both of few
    bits) comes out unchanged at any level count even with sigma_color = +inf; and a NaN painted on the background never reaches a hit
    pixel (it would through w·e_q = 0·NaN if the tap were weighted 0 instead of skipped)."""
    h, w = 30, 30
    index, normal, point = flat_guides(h, w)
    index[:] = -1
    index[8:20, 5:23] = 3
    normal[index < 0] = 0
    point[index < 0] = 0
    rgb = np.empty((h, w, 3), np.float32)
    rgb[:] = (0.5, 0.75, 1.0)
    rgb[index >= 0] = (2, 0.25, 0.0625)
    for levels in (1, 4, 8):
        assert np.array_equal(run(rgb, index, normal, point, levels=levels, sigma_color=INF), rgb)
    rgb2 = rgb.copy()
    rgb2[0, 0] = np.nan
    out = run(rgb2, index, normal, point, levels=5, sigma_color=INF)
    assert np.array_equal(out[index >= 0], rgb[index >= 0])
    assert np.isnan(out[index < 0]).any()
    # background filters among itself: an impulse on the background spreads over background pixels only
    rgb3 = np.zeros((h, w, 3), np.float32)
    rgb3[7, 10] = 1  # just above the hit region
    out = run(rgb3, index, normal, point, levels=2, sigma_color=INF)
    assert (out[index >= 0] == 0).all() and (out[index < 0] > 0).sum() > 3 * 9


def test_demodulation_returns_the_albedo_edges_exactly():
    """c = a·E with a checkerboard albedo a in {0.75, 0.25} (per channel variants) and irradiance E.  Where E is constant (0.625):
    c = a·E is exact (few bits), e = c / m with m = max(a, 2^-8) = a is the exactly representable 0.625, the filter sees a constant
    image (fixed point, previous test), and the result e·m = 0.625·a = c bit for bit: the checker's edges are back, where a filter
    of c itself would have blurred them (checked too).  In the right part E ramps and e is smooth: the output stays within the ramp's
    range times a, and differs from the input."""
    h, w = 32, 48
    index, normal, point = flat_guides(h, w)
    gx, gy = np.meshgrid(np.arange(w), np.arange(h))
    check = ((gx // 3 + gy // 3) % 2).astype(bool)
    albedo = np.where(check[..., None], np.float32([0.75, 0.5, 0.25]), np.float32([0.25, 0.75, 1.0])).astype(np.float32)
    E = np.full((h, w), 0.625, np.float32)
    E[:, 24:] = 0.625 + (gx[:, 24:] - 23) * np.float32(0.03125)
    rgb = albedo * E[..., None]
    out = run(rgb, index, normal, point, albedo, levels=3, sigma_color=INF)
    # pixels all of whose (up to) 3 levels of taps stay in the constant part: 2·(1 + 2 + 4) = 14 columns from the ramp
    assert np.array_equal(out[:, :10], rgb[:, :10])
    plain = run(rgb, index, normal, point, None, levels=3, sigma_color=INF)
    assert not np.array_equal(plain[:, :10], rgb[:, :10])
    ramp = out[:, 30:] / albedo[:, 30:]
    assert (ramp >= 0.625).all() and (ramp <= E.max() * (1 + 1e-6)).all() and not np.array_equal(out[:, 30:], rgb[:, 30:])
    # the floor: an albedo channel of 0 divides by 2^-8, not by 0, and a black surface stays black
    albedo0 = albedo.copy()
    albedo0[5:9, 2:6] = 0
    rgb0 = albedo0 * E[..., None]
    out0 = run(rgb0, index, normal, point, albedo0, levels=3, sigma_color=INF)
    assert np.isfinite(out0).all()
    # background pixels ignore the albedo they are given (m = 1)
    index_bg = index.copy()
    index_bg[:] = -1
    albedo_bg = np.full_like(albedo, 0.5)
    const = np.full((h, w, 3), 0.75, np.float32)
    assert np.array_equal(run(const, index_bg, normal, point, albedo_bg, levels=2), const)


# ---- the C ABI's refusals: every one decided before the handle is looked at, none touches a device ---------------------------
def _run_rc(lib, prm=None, rgb_in=1 << 20, out=2 << 20, g="ok", handle=None):
    o = capi.QueryOutputs(index=1 << 12, normal=2 << 12, point=3 << 12, albedo=4 << 12)
    if g not in ("ok", None):
        for k in g:
            setattr(o, k, None)
    return lib.rayz_hip_denoiser_run(handle, C.byref(prm) if prm is not None else None, C.c_void_p(rgb_in), C.byref(o) if g is not None else None,
                                     C.c_void_p(out), None)


def _params(**kw):
    return capi.DenoiseParams(**{**capi.DENOISE_DEFAULTS, **kw})


def test_denoiser_refusals_without_a_device(built):
    lib = capi.load()
    h = C.c_void_p()
    for wd, ht in ((0, 10), (10, 0), (0, 0)):
        assert lib.rayz_hip_denoiser_create(-1, wd, ht, C.byref(h)) == capi.ERR_BAD_ARG and not h.value
        assert b"zero size" in lib.rayz_hip_last_error()
    assert lib.rayz_hip_denoiser_create(-1, 8, 8, None) == capi.ERR_BAD_ARG
    bad = [
        (_params(levels=9), b"levels"), (_params(normal_power_log2=17), b"normal_power_log2"),
        (_params(sigma_color=0.0), b"sigma_color"), (_params(sigma_color=-1.0), b"sigma_color"), (_params(sigma_color=float("nan")), b"sigma_color"),
        (_params(sigma_color=1e-30), b"sigma_color"),  # positive, but its f32 square is 0: the colour term would divide 0 by 0
        (_params(sigma_plane=0.0), b"sigma_plane"), (_params(sigma_plane=-0.5), b"sigma_plane"), (_params(sigma_plane=float("nan")), b"sigma_plane"),
        (_params(flags=8), b"flag"), (_params(flags=0x80000001), b"flag"),
        (_params(flags=2), b"flag"), (_params(flags=4 | capi.DENOISE_ALBEDO), b"flag"),
    ]
    for prm, word in bad:
        assert _run_rc(lib, prm) == capi.ERR_BAD_ARG, word
        assert word in lib.rayz_hip_last_error(), (word, lib.rayz_hip_last_error())
    assert _run_rc(lib, _params(), rgb_in=None) == capi.ERR_BAD_ARG
    assert _run_rc(lib, _params(), out=None) == capi.ERR_BAD_ARG
    assert _run_rc(lib, _params(), g=None) == capi.ERR_BAD_ARG
    for k in ("index", "normal", "point", "albedo"):
        assert _run_rc(lib, _params(), g=(k,)) == capi.ERR_BAD_ARG, k
        assert _run_rc(lib, None, g=(k,)) == capi.ERR_BAD_ARG, k  # params == NULL: the defaults demodulate, so albedo is required
    # albedo may be missing when the flag is off; everything accepted: what is left to refuse is the handle
    assert _run_rc(lib, _params(flags=0), g=("albedo",)) == capi.ERR_STATE
    assert _run_rc(lib, _params(levels=0, sigma_color=INF, sigma_plane=INF)) == capi.ERR_STATE
    assert _run_rc(lib, _params(levels=8, normal_power_log2=16)) == capi.ERR_STATE
    assert _run_rc(lib, None) == capi.ERR_STATE
    junk = (C.c_uint32 * 16)()
    assert _run_rc(lib, None, handle=C.cast(junk, C.c_void_p)) == capi.ERR_STATE
    assert lib.rayz_hip_denoiser_destroy(C.cast(junk, C.c_void_p)) == capi.ERR_STATE
    assert lib.rayz_hip_denoiser_destroy(None) == capi.OK
    n, ms = C.c_uint32(), (C.c_float * 9)()
    assert lib.rayz_hip_denoiser_timing(None, C.byref(n), ms, 9) == capi.ERR_STATE
    assert lib.rayz_hip_denoiser_timing(C.cast(junk, C.c_void_p), C.byref(n), ms, 9) == capi.ERR_STATE
    # the staging knob (which levels use LDS: scheduling, never a value) takes the strides the staged form exists for
    try:
        for bad in (3, 5, 8, 1 << 20):
            assert lib.rayz_hip_debug_set(capi.DEBUG_DENOISE_LDS_STRIDE, bad) == capi.ERR_BAD_ARG and b"DENOISE_LDS_STRIDE" in lib.rayz_hip_last_error()
        for good in (0, 1, 2, 4, -1):
            assert lib.rayz_hip_debug_set(capi.DEBUG_DENOISE_LDS_STRIDE, good) == capi.OK
    finally:
        lib.rayz_hip_debug_set(capi.DEBUG_DENOISE_LDS_STRIDE, -1)


def test_create_without_a_device_is_an_error(built):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the gpu tests")
    lib = capi.load()
    h = C.c_void_p()
    assert lib.rayz_hip_denoiser_create(-1, 16, 16, C.byref(h)) == capi.ERR_NO_DEVICE and not h.value
    assert lib.rayz_hip_denoiser_create(0, 16, 16, C.byref(h)) == capi.ERR_NO_DEVICE and not h.value


# ---- quality ------------------------------------------------------------------------------------------------------------------
def cpu_gbuffer(oracle, t):
    """The getRay(px, py, null) G-buffer of every pixel from the oracle's pieces (tests/query_reference.py): index, normal, point,
    albedo as float32 frames."""
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    w, h = p.width, p.height
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    rec = np.zeros((w * h, capi.KAT_IN_STRIDE))
    for k, f in enumerate([cam.look_from, cam.px_du, cam.px_dv, cam.px_origin, cam.defocus_u, cam.defocus_v]):
        rec[:, 3 * k:3 * k + 3] = list(f)
    rec[:, 18], rec[:, 19], rec[:, 20], rec[:, 21] = cam.defocus, px.ravel(), py.ravel(), -1
    kr = oracle.kat_b(capi.KAT_GET_RAY, rec, qr.F32)
    rays = np.zeros((w * h, 8))
    rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7] = kr[:, 0:3], kr[:, 3:6], kr[:, 6], np.inf
    idx, _, out, _ = qr.brute_force(oracle, sd, rays, qr.TMIN, qr.F32)
    _, _, _, sm, _, _ = qr.pool_arrays(sd)
    albedo = np.zeros((w * h, 3))
    for k in np.nonzero(idx >= 0)[0]:
        albedo[k] = qr.albedo_of(oracle, sd, int(sm[idx[k]]), out[k, 2:5], qr.F32)
    f = lambda a: a.astype(np.float32).reshape(h, w, -1)  # noqa: E731
    return idx.astype(np.int32).reshape(h, w), f(out[:, 5:8]), f(out[:, 2:5]), f(albedo)


def test_denoised_4spp_frame_is_nearer_to_256spp_than_the_noisy_one(oracle):
    """randomBouncing at 96x54: the oracle's (mode B) 4-spp frame, denoised by the mirror with the default parameters and the
    oracle's first-hit G-buffer, against the oracle's 256-spp frame.  The condition is MSE(denoised) < MSE(noisy); the measured
    ratio is recorded in DESIGN.md §6, it is not a threshold."""
    t = tracer.randomBouncing(96, seed=7)
    t.max_bounces = 12
    t.set_gpu(render_seed=11)
    index, normal, point, albedo = cpu_gbuffer(oracle, t)
    frames = {}
    for spp in (4, 256):
        t.samples_per_px = spp
        frames[spp], _ = oracle.render_b(t.scene_desc(), t.camera_desc(), t.params())
    noisy, clean = frames[4].astype(np.float32), frames[256].astype(np.float64)
    den = denoise_ref.denoise(noisy, index, normal, point, albedo, **denoise_ref.DEFAULTS)
    mse = lambda a: float(((a.astype(np.float64) - clean) ** 2).mean())  # noqa: E731
    print(f"MSE noisy {mse(noisy):.6e} denoised {mse(den):.6e} ratio {mse(den) / mse(noisy):.4f}")
    assert np.isfinite(den).all()
    assert mse(den) < mse(noisy)
