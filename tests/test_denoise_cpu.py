"""The à-trous denoiser without a GPU: hand-derived known answers on the CPU restatement
(tests/denoise_mirror.cpp, which the GPU tests hold the kernels to bit for bit) — with weights of 0 and 1 first, then the exact
rational cases of tests/denoise_cases.py, whose weights are proper fractions, and a float64 statement of §4.11 on general guides
(tests/denoise_f64.py) that the mirror must stay within a derived bound of and every listed misreading must leave — then the
C ABI's refusals, and the quality condition — a denoised 4-spp frame of the oracle is nearer to its 256-spp frame than the noisy one."""
import ctypes as C
import functools
import itertools
import os
from concurrent.futures import ThreadPoolExecutor
from fractions import Fraction as F

import numpy as np
import pytest

import denoise_cases
import denoise_f64
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


# ---- exact answers with weights that are neither 0 nor 1 (tests/denoise_cases.py) ----------------------------------------------
CASES = {c.name: c for c in denoise_cases.cases()}


def test_the_rational_evaluator_gives_the_closed_forms_written_by_hand():
    """denoise_cases.exact() is §4.11 in Fractions; every case's `hand` is the closed form of its comment with literal weights.  They
    must agree as rationals, before any rounding.  Two of them once more as bare numbers (base case, L = 3, k = 1): wn = 1/4;
    out_A = w / (9/64 + w) with w = 3/128·1/4·1/4·1/4 = 3/8192, i.e. 3 / (1152 + 3) = 1/385; out_B = c / (c + w') with c = 9/64·1/16 =
    1152/131072 and w' = 3/128·1/4·49/64·1/4 = 147/131072, i.e. 1152/1299 = 384/433.  And the 3x3 frame's centre pixel (and 7 of the
    other 8) has nine pairwise different, nonzero weights."""
    for c in CASES.values():
        if c.general:
            assert denoise_cases.exact(c) == c.hand, c.name
    b = CASES["base-row-L3-k1"]
    assert b.hand[(0, 0)] == [F(1, 385)] * 3 and b.hand[(0, 8)] == [F(384, 433)] * 3
    wts = {}
    denoise_cases.exact(CASES["nine-weights-3x3"], wts)
    assert len(wts) == 9 and len(set(wts[(1, 1)])) == 9 and 0 not in wts[(1, 1)]
    assert sum(len(set(v)) == 9 and 0 not in v for v in wts.values()) >= 8


@pytest.mark.parametrize("name", sorted(CASES))
def test_the_mirror_gives_the_rational_answer_bit_for_bit(name):
    """Every hit pixel of every case of tests/denoise_cases.py (each derived there): the mirror's f32 equals the rational S / W rounded
    once (then ×m, exact).  No NaN of the background may have reached a hit."""
    c = CASES[name]
    c.check(run(c.rgb, c.index, c.normal, c.point, c.albedo, **c.params), "mirror")


def test_a_zero_normal_makes_nan_at_its_own_pixel_only():
    """§4.11 promises W > 0 for unit normals only.  A hit with the normal (0,0,0): its own W is 0 and its output 0/0 = NaN; as a
    NEIGHBOUR its weight is an honest 0 with finite e_q, so no other pixel's W or S changes (denoise_cases.zero_normal derives every
    value: W_p = A(x)·A(y) - k·k of the missing tap).  Recorded behaviour, one level: a second level would read the NaN."""
    c = CASES["zero-normal-5x5"]
    out = run(c.rgb, c.index, c.normal, c.point, None, **c.params)
    assert np.isnan(out[2, 2]).all() and np.isnan(out).sum() == 3
    c.check(out, "mirror")
    assert out[0, 0, 0] == np.float32((1 / 4 * 3 / 8) / (121 / 256 - 1 / 256))  # I = (0,1) seen from (0,0): k[1]·k[0] / (A(0)^2 - k[2]^2)


# ---- the float64 reference on general guides ------------------------------------------------------------------------------------
F64_SIZES = ((63, 65, 6365), (131, 77, 5))  # (width, height, seed of synthetic())
F64_LEVELS = (1, 3, 5, 8)
F64_STATES = [dict(flags=f, sigma_color=sc, sigma_plane=0.3) for f, sc in itertools.product((denoise_ref.ALBEDO, 0), (0.4, INF))] + [
    {k: denoise_ref.DEFAULTS[k] for k in ("flags", "sigma_color", "sigma_plane")}]
F64_COMBOS = [dict(st, normal_power_log2=k) for k in (0, 6) for st in F64_STATES]
EXCLUDED_CAP = 0.001
POOL = max(1, min(8, os.cpu_count() or 1))


@functools.lru_cache(maxsize=None)
def f64_inputs(size):
    w, h, seed = F64_SIZES[size]
    return denoise_cases.synthetic(w, h, seed)


@functools.lru_cache(maxsize=None)
def f64_config(size, combo):
    """(mirror results, reference results with bound) for levels F64_LEVELS: computed once, shared, never changed."""
    inp, prm = f64_inputs(size), F64_COMBOS[combo]
    mir = denoise_ref.denoise(*inp, levels=8, each_level=True, threads=1, **prm)
    ref = denoise_f64.denoise_f64(*inp, levels=8, want_levels=F64_LEVELS, bound=True, **prm)
    return {L: mir[L - 1] for L in F64_LEVELS}, ref


def _tag(size, combo, L):
    p = F64_COMBOS[combo]
    return f"{F64_SIZES[size][0]}x{F64_SIZES[size][1]} L={L} flags={p['flags']} sc={p['sigma_color']} sp={p['sigma_plane']} k={p['normal_power_log2']}"


def test_the_mirror_is_within_the_derived_bound_of_the_f64_reference():
    """synthetic() guides at 63x65 and 131x77; 1, 3, 5, 8 levels; the four (flag, sigma_color) states at sigma_plane 0.3 and the
    defaults; normal_power_log2 0 and 6: 80 configurations.  Tolerance, per value: denoise_f64's bound — derived in that module's
    docstring from the rounding count of a tap, |δout| <= Σ_q |δw_q|·|e_q − out| / W plus the propagated input error and the 50
    roundings of the sums, every quantity the f64 reference's own, DOUBLED for the second-order terms the first-order propagation
    drops.  The relative error of wn grows 2^k-fold under the squarings (2^6·3u ≈ 1.1e-5 at k = 6), which is why k stops at 6 here.
    Pixels whose reference W is below 2^-20 at some level are excluded; at most 0.1 % of a frame may be (measured: none — a hit's
    centre tap alone gives W >= 9/64·(n.n)^64 ≈ 0.14 for the unit normals of these guides).  The measured errors are printed and
    recorded in DESIGN.md §3; they are not thresholds."""
    jobs = list(itertools.product(range(len(F64_SIZES)), range(len(F64_COMBOS))))
    with ThreadPoolExecutor(POOL) as pool:
        list(pool.map(lambda a: f64_config(*a), jobs))
    worst = (0.0, 0.0, "")
    for size, combo in jobs:
        mir, ref = f64_config(size, combo)
        for L in F64_LEVELS:
            out, bound, excluded = ref[L]
            assert np.isfinite(out).all() and np.isfinite(bound).all(), _tag(size, combo, L)
            assert excluded.mean() <= EXCLUDED_CAP, (_tag(size, combo, L), int(excluded.sum()))
            err = np.abs(mir[L].astype(np.float64) - out)
            keep = ~excluded[..., None] & np.ones(3, bool)
            ratio = float((err[keep] / bound[keep]).max())
            print(f"mirror vs f64: {_tag(size, combo, L)}: max |err| {err[keep].max():.3e}, max err/bound {ratio:.4f}, excluded {int(excluded.sum())}")
            worst = max(worst, (ratio, float(err[keep].max()), _tag(size, combo, L)))
            assert (err[keep] <= bound[keep]).all(), (_tag(size, combo, L), ratio)
    print(f"mirror vs f64, worst: err/bound {worst[0]:.4f} (|err| {worst[1]:.3e}) at {worst[2]}")


def test_every_misreading_of_the_f64_reference_is_rejected():
    """Each of denoise_f64.MISREADINGS, switched into the f64 reference, must differ from the MIRROR by more than the bound of the
    test above (the reference-as-written's, at the same configuration) at some value of some configuration — were mirror and kernel
    to adopt that misreading together, the test above would fail by the same margin.  Run at 63x65 over all 40 configurations there
    (the larger frame adds time, not cases).  A misreading that a configuration cannot show (4^l at one level, the colour term at
    sigma_color = +inf, the floor without demodulation, wn^(k+1) at k = 0) is simply not caught THERE; the condition is one catch.
    `bg_weighted_zero` changes no value on a finite frame (it adds 0 to W and fma(0, e_q, S) = S), so it alone runs on the same
    guides with a NaN sky: the mirror keeps every hit pixel within the bound of the reference, the misreading turns hits to NaN."""
    size = 0
    inp = f64_inputs(size)
    hit = inp[1] >= 0
    sky = list(inp)
    sky[0] = inp[0].copy()
    sky[0][~hit] = np.nan

    def one(combo):
        prm = F64_COMBOS[combo]
        mir, ref = f64_config(size, combo)
        mir_sky = denoise_ref.denoise(*sky, levels=8, each_level=True, threads=1, **prm)
        rows = {}
        for name in denoise_f64.MISREADINGS:
            on_sky = name == "bg_weighted_zero"
            got = denoise_f64.denoise_f64(*(sky if on_sky else inp), levels=8, want_levels=F64_LEVELS, misread=name, **prm)
            for L in F64_LEVELS:
                out, bound, excluded = ref[L]
                keep = hit & ~excluded
                m = mir_sky[L - 1] if on_sky else mir[L]
                if on_sky:  # the mirror itself is unharmed by the sky's NaN, to the same bound
                    assert (np.abs(m[keep].astype(np.float64) - out[keep]) <= bound[keep]).all(), (name, _tag(size, combo, L))
                with np.errstate(invalid="ignore"):
                    ratio = np.abs(m[keep].astype(np.float64) - got[L][keep]) / bound[keep]
                rows[(name, L)] = float("inf") if np.isnan(ratio).any() else float(ratio.max())  # a NaN is outside any tolerance
        return rows

    with ThreadPoolExecutor(POOL) as pool:
        rows = list(pool.map(one, range(len(F64_COMBOS))))
    for name in denoise_f64.MISREADINGS:
        for combo, r in enumerate(rows):
            for L in F64_LEVELS:
                print(f"misreading {name}: {_tag(size, combo, L)}: max |misread - mirror| / bound {r[(name, L)]:.4g}")
        caught = [r[(name, L)] for r in rows for L in F64_LEVELS if r[(name, L)] > 1]
        print(f"misreading {name}: caught in {len(caught)} of {len(rows) * len(F64_LEVELS)} configurations; smallest catch {min(caught, default=0):.4g} x bound, "
              f"largest {max(caught, default=0):.4g} x bound")
        assert caught, f"the misreading {name} stays within the tolerance of the mirror on every input"


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
