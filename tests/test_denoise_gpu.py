"""The à-trous denoiser on the GPU (rayz_hip_denoiser_*, `render.Denoiser`): every value of every frame equals the CPU restatement of
DESIGN.md §4.11 (tests/denoise_mirror.cpp) bit for bit — synthetic guides at sizes that are no multiple of a tile and smaller than a
halo, every level count, both flag states, the colour term on and off, in place and out of place, every staging form of the levels,
and real G-buffers with rendered 4-spp frames; plus stream ordering after a progressive preview and repeatability on one handle.
Two comparisons do not go through the mirror: the exact rational cases of tests/denoise_cases.py, bit for bit, and the float64
statement of §4.11 (tests/denoise_f64.py) within its derived bound."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import denoise_cases
import denoise_f64
import denoise_ref
from denoise_cases import synthetic
from helpers import assert_images_equal
from rayz_amd import capi, render, tracer

pytestmark = pytest.mark.gpu

INF = float("inf")
BVH = capi.TRAVERSAL_BVH
STAGING = (-1, 0, 1, 2, 4)  # RAYZ_DEBUG_DENOISE_LDS_STRIDE: the built-in choice; no level staged in LDS; strides up to 1 / 2 / 4 staged
SMALL = [(1, 1), (1, 7), (7, 1), (5, 3), (63, 65), (257, 130)]  # (width, height)


def to_gbuffer(index, normal, point, albedo):
    g = render.QueryResult()
    g.index, g.normal, g.point, g.albedo = (torch.from_numpy(a).cuda() for a in (index, normal, point, albedo))
    return g


def gpu_run(dn, rgb, g, in_place, staging=-1, **prm):
    x = torch.from_numpy(rgb).cuda()
    render.debug_set(capi.DEBUG_DENOISE_LDS_STRIDE, staging)
    try:
        out = dn.run(x, g, out=x if in_place else None, **prm)
    finally:
        render.debug_set(capi.DEBUG_DENOISE_LDS_STRIDE, -1)
    torch.cuda.synchronize()
    if not in_place:
        assert np.array_equal(x.cpu().numpy().view(np.uint32), rgb.view(np.uint32)), "an out-of-place run changed its input"
    return out.cpu().numpy()


@pytest.mark.parametrize("w,h", SMALL)
def test_device_equals_the_mirror_on_small_frames(gpu, w, h):
    """The whole product levels x flag x sigma_color x placement; the staging cycles through STAGING (5 settings against 16 runs per
    state: every level count meets every setting over the four states)."""
    rgb, index, normal, point, albedo = synthetic(w, h, 100 * w + h)
    g = to_gbuffer(index, normal, point, albedo)
    dn = render.Denoiser(w, h)
    staging = itertools.cycle(STAGING)
    for flag, sc in itertools.product((capi.DENOISE_ALBEDO, 0), (0.4, INF)):
        want = denoise_ref.denoise(rgb, index, normal, point, albedo, levels=8, flags=flag, sigma_color=sc, sigma_plane=0.3, each_level=True)
        for levels, in_place in itertools.product(range(1, 9), (False, True)):
            got = gpu_run(dn, rgb, g, in_place, staging=next(staging), levels=levels, flags=flag, sigma_color=sc, sigma_plane=0.3)
            assert_images_equal(got, want[levels - 1], f"{w}x{h} L={levels} flags={flag} sigma_color={sc} in_place={in_place}")
    dn.close()


def test_every_staging_form_gives_the_same_bits(gpu):
    """Every staging setting on one input: one image (the forms differ in where a tap is fetched from, nothing else),
    at a size with partial tiles on both edges, for the other parameter values too (normal_power_log2 0 and 16, levels = 0 -> 5);
    and, with 5 levels, at 5x3 (smaller than every halo) and 45x23 (no tile multiple; a stride-4 halo crosses the frame on all sides)."""
    for w, h, states in ((131, 77, ((0, 0), (16, 3), (6, 5))), (5, 3, ((6, 5),)), (45, 23, ((6, 5),))):
        rgb, index, normal, point, albedo = synthetic(w, h, 5)
        g = to_gbuffer(index, normal, point, albedo)
        dn = render.Denoiser(w, h)
        for npl, levels in states:
            want = denoise_ref.denoise(rgb, index, normal, point, albedo, levels=levels, normal_power_log2=npl)
            for st in STAGING:
                got = gpu_run(dn, rgb, g, False, staging=st, levels=levels, normal_power_log2=npl)
                assert_images_equal(got, want, f"{w}x{h} npl={npl} levels={levels} staging={st}")
        dn.close()


def test_device_equals_the_mirror_at_1920x1080(gpu):
    """Every level count 1..8 for the four (flag, sigma_color) states; placement and staging form alternate."""
    w, h = 1920, 1080
    rgb, index, normal, point, albedo = synthetic(w, h, 9)
    g = to_gbuffer(index, normal, point, albedo)
    dn = render.Denoiser(w, h)
    staging = itertools.cycle(STAGING)
    place = itertools.cycle((False, True))
    for flag, sc in itertools.product((capi.DENOISE_ALBEDO, 0), (0.5, INF)):
        want = denoise_ref.denoise(rgb, index, normal, point, albedo, levels=8, flags=flag, sigma_color=sc, each_level=True)
        for levels in range(1, 9):
            got = gpu_run(dn, rgb, g, next(place), staging=next(staging), levels=levels, flags=flag, sigma_color=sc)
            assert_images_equal(got, want[levels - 1], f"1920x1080 L={levels} flags={flag} sigma_color={sc}")
    dn.close()


def test_device_gives_the_rational_answers_bit_for_bit(gpu):
    """Every case of tests/denoise_cases.py (two hits 2^L apart with proper-fraction weights, L = 1..8; column, diagonal, stride 1;
    wn underflowing, back-facing, d2 == 0, u clamped; demodulation with the floor; nine different weights in a 3x3 frame) under every
    staging setting, out of place and in place, held to the RATIONAL expectation (Fractions, rounded once) directly — not to the
    mirror.  The NaN of the background pixels must not reach a hit."""
    handles = {}
    for c in denoise_cases.cases():
        if c.name.startswith("zero-normal"):
            continue  # what §4.11 does not promise has its own test below
        h, w = c.index.shape
        dn = handles.get((w, h)) or handles.setdefault((w, h), render.Denoiser(w, h))
        g = to_gbuffer(c.index, c.normal, c.point, c.albedo if c.albedo is not None else np.zeros_like(c.normal))
        for st, in_place in itertools.product(STAGING, (False, True)):
            c.check(gpu_run(dn, c.rgb, g, in_place, staging=st, **c.params), f"device staging={st} in_place={in_place}")
    for dn in handles.values():
        dn.close()


def test_a_zero_normal_makes_nan_at_its_own_pixel_only(gpu):
    """The device on the input of test_denoise_cpu.py's test of the same name: a hit whose normal is (0,0,0) gets 0/0 = NaN at its own
    pixel after one level; every other pixel has the rational value derived in denoise_cases.zero_normal, as the mirror has."""
    c = next(c for c in denoise_cases.cases() if c.name.startswith("zero-normal"))
    h, w = c.index.shape
    dn = render.Denoiser(w, h)
    g = to_gbuffer(c.index, c.normal, c.point, np.zeros_like(c.normal))
    for st in (-1, 0):
        out = gpu_run(dn, c.rgb, g, False, staging=st, **c.params)
        assert np.isnan(out[2, 2]).all() and np.isnan(out).sum() == 3
        c.check(out, f"device staging={st}")
    dn.close()


@pytest.mark.parametrize("w,h,seed", [(63, 65, 6365), (131, 77, 5)])
def test_device_is_within_the_derived_bound_of_the_f64_reference(gpu, w, h, seed):
    """The device against tests/denoise_f64.py DIRECTLY, within the per-value bound derived in that module (and used, with the same
    exclusion cap, by test_denoise_cpu.py): 1, 5 and 8 levels with the default parameters and with one state without demodulation.
    Redundant with device == mirror by design: this comparison survives an edit of the mirror."""
    inp = synthetic(w, h, seed)
    g = to_gbuffer(*inp[1:])
    dn = render.Denoiser(w, h)
    levels = (1, 5, 8)
    for prm in (dict(), dict(flags=0, sigma_color=0.4, sigma_plane=0.3)):
        ref = denoise_f64.denoise_f64(*inp, **{**denoise_ref.DEFAULTS, **prm, "levels": 8}, want_levels=levels, bound=True)
        for L in levels:
            out, bound, excluded = ref[L]
            assert excluded.mean() <= 0.001, (L, int(excluded.sum()))
            got = gpu_run(dn, inp[0], g, False, levels=L, **prm).astype(np.float64)
            err = np.abs(got - out)[~excluded]
            print(f"device vs f64: {w}x{h} L={L} {prm}: max |err| {err.max():.3e}, max err/bound {(err / bound[~excluded]).max():.4f}")
            assert (err <= bound[~excluded]).all(), (w, h, L, prm, float((err / bound[~excluded]).max()))
    dn.close()


def _scene(name):
    if name == "threeSpheres":
        t = tracer.threeSpheres(160, seed=3)
    elif name == "randomBouncing":
        t = tracer.randomBouncing(200, -5, 5, seed=5)
    else:
        t = tracer.triangleMesh(144, 24, seed=1)
    t.samples_per_px, t.max_bounces = 4, 8
    t.set_gpu(render_seed=17, chunk_spp=4)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    p.traversal, p.tmin = BVH, 1e-3
    return t, sd, cam, p


@pytest.mark.parametrize("name", ["threeSpheres", "randomBouncing", "triangleMesh"])
def test_real_gbuffers_and_rendered_frames(gpu, name):
    t, sd, cam, p = _scene(name)
    ds = render.DeviceScene(sd)
    frame = torch.empty((p.height, p.width, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ds.render_into(cam, p, frame.data_ptr())
    ds.sync()
    g = ds.gbuffer(cam, p)
    ds.query_sync()
    host = [getattr(g, k).cpu().numpy() for k in ("index", "normal", "point", "albedo")]
    assert (host[0] >= 0).any()
    rgb = frame.cpu().numpy()
    dn = render.Denoiser(p.width, p.height)
    for prm in (dict(), dict(levels=3, sigma_color=INF, flags=0), dict(levels=8, sigma_color=0.2, sigma_plane=0.1, normal_power_log2=3)):
        want = denoise_ref.denoise(rgb, *host, **{**denoise_ref.DEFAULTS, **prm})
        got = dn.run(frame, g, **prm)
        torch.cuda.synchronize()
        assert_images_equal(got.cpu().numpy(), want, f"{name} {prm}")
        assert not np.array_equal(want, rgb)
    dn.close()
    ds.close()


def test_a_progressive_preview_is_denoised_as_its_copy_is(gpu):
    """Stream ordering against the library's stream.  Through the C ABI, with a NULL stream everywhere and NO host synchronisation
    in between (the Python layer would synchronise the device before each call): a progressive step that writes the preview, the
    camera query that writes the G-buffer, and the denoiser run that reads both are enqueued back to back.  The run must see both
    complete — which it does only if it is enqueued on the library's stream behind them.  The result equals the denoised copy of
    the same preview and G-buffer taken after a synchronise.  16 spp in chunks of 4 at 400x225, so that the step and the query are
    still in flight when the run is enqueued."""
    lib = capi.load()
    t = tracer.randomBouncing(400, -11, 11, seed=5)
    t.samples_per_px, t.max_bounces = 16, 8
    t.set_gpu(render_seed=17, chunk_spp=4)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    p.traversal, p.tmin = BVH, 1e-3
    w, h = p.width, p.height
    ds = render.DeviceScene(sd)
    dn = render.Denoiser(w, h)
    pr = ds.progressive(cam, p)
    nan = float("nan")
    preview = torch.full((h, w, 3), nan, device="cuda")
    out = torch.full((h, w, 3), nan, device="cuda")
    g = render.QueryResult._alloc((h, w), torch.float32, torch.device("cuda", 0), ("index", "normal", "point", "albedo"))
    prm = capi.DenoiseParams(**capi.DENOISE_DEFAULTS)
    seen = 0
    while not pr.done:
        preview.fill_(nan), out.fill_(nan), g.normal.fill_(nan), g.point.fill_(nan), g.albedo.fill_(nan), g.index.fill_(-1)
        torch.cuda.synchronize()
        o = g._outputs()
        rcs = (lib.rayz_hip_progressive_step(pr._h, 0, C.c_void_p(preview.data_ptr()), None),
               lib.rayz_hip_scene_query_camera(ds._h, C.byref(cam), C.byref(p), C.byref(o), None),
               lib.rayz_hip_denoiser_run(dn._h, C.byref(prm), C.c_void_p(preview.data_ptr()), C.byref(o), C.c_void_p(out.data_ptr()), None))
        assert rcs == (capi.OK, capi.OK, capi.OK), (rcs, lib.rayz_hip_last_error())
        torch.cuda.synchronize()
        ds.query_sync()
        pr.stats()
        assert torch.isfinite(preview).all() and torch.isfinite(out).all() and (g.index >= 0).any()
        again = dn.run(preview.clone(), g)
        torch.cuda.synchronize()
        assert_images_equal(out.cpu().numpy(), again.cpu().numpy(), f"preview after {pr.samples_done} samples")
        assert not torch.equal(out, preview)
        seen += 1
    assert seen == 4
    pr.close()
    dn.close()
    ds.close()


def test_timing_reports_the_levels_of_the_last_run(gpu):
    w, h = 640, 360
    rgb, index, normal, point, albedo = synthetic(w, h, 3)
    g = to_gbuffer(index, normal, point, albedo)
    dn = render.Denoiser(w, h)
    with pytest.raises(capi.RayzHipError, match="no denoiser run"):
        dn.timing()
    for levels in (1, 5, 8):
        gpu_run(dn, rgb, g, False, levels=levels)
        pack, lv = dn.timing()
        assert len(lv) == levels and pack > 0 and all(0 < x < 1000 for x in lv), (pack, lv)
    # a run on a stream the caller then destroys: the next run and close() wait on the handle's own event, not on that stream
    x = torch.from_numpy(rgb).cuda()
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    a = dn.run(x, g, stream=s.cuda_stream)
    del s
    b = dn.run(x, g)
    torch.cuda.synchronize()
    assert_images_equal(b.cpu().numpy(), a.cpu().numpy(), "run after a run on a released stream")
    dn.close()


def test_two_runs_on_one_handle_are_identical_and_sizes_are_checked(gpu):
    w, h = 300, 170
    rgb, index, normal, point, albedo = synthetic(w, h, 77)
    g = to_gbuffer(index, normal, point, albedo)
    dn = render.Denoiser(w, h)
    a = gpu_run(dn, rgb, g, False)
    other = gpu_run(dn, rgb[::-1].copy(), g, False, levels=2)  # a different run in between leaves nothing behind
    b = gpu_run(dn, rgb, g, False)
    assert_images_equal(b, a, "second run on one handle")
    assert not np.array_equal(other, a)
    # a caller's stream: ordered by the caller
    s = torch.cuda.Stream()
    x = torch.from_numpy(rgb).cuda()
    torch.cuda.synchronize()
    c = dn.run(x, g, stream=s.cuda_stream)
    s.synchronize()
    assert_images_equal(c.cpu().numpy(), a, "run on a caller's stream")
    with pytest.raises(ValueError, match="must be"):
        dn.run(x[:, :-1].contiguous(), g)
    with pytest.raises(ValueError, match="float32"):
        dn.run(x.double(), g)
    with pytest.raises(ValueError, match="GPU memory"):
        dn.run(x.cpu(), g)
    with pytest.raises(ValueError, match="unknown denoise parameter"):
        dn.run(x, g, sigma=1.0)
    with pytest.raises(capi.RayzHipError, match="levels"):
        dn.run(x, g, levels=9)
    dn.close()
