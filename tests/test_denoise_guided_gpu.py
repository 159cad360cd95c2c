"""The variance-guided denoiser on the GPU (rayz_hip_denoiser_run_guided, `render.Denoiser.run_guided`): every
colour and every variance equals the CPU restatement (tests/denoise_guided_mirror.cpp) bit for bit — synthetic guides and variances
spanning 0, tiny, large, +inf and NaN, at sizes that are no tile multiple and smaller than a halo, 1, 3 and 5 levels, both flag
states, with and without the variance output, every staging setting of the levels; the hand-derived exact answers of
tests/denoise_guided_cases.py; in place and repeatable; the unguided mode undisturbed on the same handle; and end to end from a
tracked progressive handle."""
import itertools

import numpy as np
import pytest
import torch

import denoise_guided_cases
import denoise_guided_ref
import denoise_ref
from denoise_cases import synthetic
from denoise_guided_cases import guided_variance
from rayz_amd import capi, render, tracer

pytestmark = pytest.mark.gpu

INF = float("inf")
STAGING = (0, 1, 2, 4)  # RAYZ_DEBUG_DENOISE_LDS_STRIDE: no level staged in LDS; strides up to 1 / 2 / 4 staged
SIZES = [(1, 1), (5, 3), (33, 9), (45, 23), (97, 41)]  # (width, height)


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ; first at {bad[:5].tolist()}: " \
                          f"{[(got[tuple(b)], want[tuple(b)]) for b in bad[:3]]}"


def to_gbuffer(index, normal, point, albedo):
    g = render.QueryResult()
    g.index, g.normal, g.point, g.albedo = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (index, normal, point, albedo))
    return g


def gpu_run(dn, rgb, var_rgb, g, in_place=False, var_out=True, staging=-1, **prm):
    x, v = torch.from_numpy(rgb).cuda(), torch.from_numpy(var_rgb).cuda()
    render.debug_set(capi.DEBUG_DENOISE_LDS_STRIDE, staging)
    try:
        res = dn.run_guided(x, v, g, out=x if in_place else None, var_out=var_out, **prm)
    finally:
        render.debug_set(capi.DEBUG_DENOISE_LDS_STRIDE, -1)
    torch.cuda.synchronize()
    out, vo = res if var_out else (res, None)
    if not in_place:
        assert np.array_equal(x.cpu().numpy().view(np.uint32), rgb.view(np.uint32)), "an out-of-place run changed its input"
    assert np.array_equal(v.cpu().numpy().view(np.uint32), var_rgb.view(np.uint32)), "the run changed the variance it was given"
    return out.cpu().numpy(), None if vo is None else vo.cpu().numpy()


@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_the_mirror(gpu, w, h):
    """levels {1, 3, 5} x albedo on / off x variance output on / off; placement and staging cycle (with the built-in choice, -1)."""
    rgb, index, normal, point, albedo = synthetic(w, h, 100 * w + h)
    var = guided_variance(rgb, w + h)
    g = to_gbuffer(index, normal, point, albedo)
    dn = render.Denoiser(w, h)
    staging = itertools.cycle((-1,) + STAGING)
    place = itertools.cycle((False, True))
    for flag in (capi.DENOISE_ALBEDO, 0):
        want = denoise_guided_ref.denoise(rgb, var, index, normal, point, albedo, levels=5, flags=flag, sigma_color=2.0, sigma_plane=0.3,
                                          var_floor=1e-4, each_level=True)
        for levels, var_out in itertools.product((1, 3, 5), (True, False)):
            st, ip = next(staging), next(place)
            got, gv = gpu_run(dn, rgb, var, g, in_place=ip, var_out=var_out, staging=st, levels=levels, flags=flag, sigma_color=2.0,
                              sigma_plane=0.3, var_floor=1e-4)
            what = f"{w}x{h} L={levels} flags={flag} var_out={var_out} staging={st} in_place={ip}"
            same_bits(got, want[levels - 1][0], what)
            assert np.isfinite(got).all(), what
            if var_out:
                same_bits(gv, want[levels - 1][1], what + " (variance)")
    dn.close()


def test_every_staging_form_gives_the_same_bits(gpu):
    """Every staging setting and the built-in choice on one input, 5 levels: at 97x41, at 5x3 (smaller than every halo) and at 45x23
    (no tile multiple; a stride-4 halo crosses the frame on all sides)."""
    assert capi.DENOISE_GUIDED_DEFAULTS["levels"] == 5
    for w, h in ((97, 41), (5, 3), (45, 23)):
        rgb, index, normal, point, albedo = synthetic(w, h, 9741)
        var = guided_variance(rgb, 11)
        g = to_gbuffer(index, normal, point, albedo)
        dn = render.Denoiser(w, h)
        want = denoise_guided_ref.denoise(rgb, var, index, normal, point, albedo, **capi.DENOISE_GUIDED_DEFAULTS)
        try:
            for st in (-1,) + STAGING:
                got, gv = gpu_run(dn, rgb, var, g, staging=st)
                same_bits(got, want[0], f"{w}x{h} staging={st}")
                same_bits(gv, want[1], f"{w}x{h} staging={st} (variance)")
        finally:
            render.debug_set(capi.DEBUG_DENOISE_LDS_STRIDE, -1)
        dn.close()


def test_device_gives_the_hand_derived_answers(gpu):
    """Every case of tests/denoise_guided_cases.py against its RATIONAL expectation directly — not through the mirror — under every
    staging setting; and a NaN, an infinite and a negative variance leave no NaN behind and equal the mirror."""
    for c in denoise_guided_cases.cases() + [x[1] for x in denoise_guided_cases.odd_variances()]:
        h, w = c.index.shape
        dn = render.Denoiser(w, h)
        g = to_gbuffer(c.index, c.normal, c.point, c.albedo if c.albedo is not None else np.zeros_like(c.normal))
        want = denoise_guided_ref.denoise(c.rgb, c.var_rgb, c.index, c.normal, c.point, c.albedo, **c.params)
        for st in (-1,) + STAGING:
            got, gv = gpu_run(dn, c.rgb, c.var_rgb, g, staging=st, **c.params)
            c.check(got, gv, f"device staging={st}")
            hit = c.index >= 0
            assert np.isfinite(got[hit]).all() and np.isfinite(gv[hit]).all(), (c.name, st)
            same_bits(got[hit], want[0][hit], f"{c.name} staging={st}")
            same_bits(gv[hit], want[1][hit], f"{c.name} staging={st} (variance)")
        dn.close()


def test_in_place_repeatable_and_the_unguided_mode_undisturbed(gpu):
    """Two guided runs on one handle are identical, in place equals out of place, and an unguided run before and after a guided one
    equals the existing mirror's bits: the variance a guided run leaves in the colour records' fourth slot reaches nothing."""
    w, h = 97, 41
    rgb, index, normal, point, albedo = synthetic(w, h, 4197)
    var = guided_variance(rgb, 5)
    g = to_gbuffer(index, normal, point, albedo)
    dn = render.Denoiser(w, h)
    x = torch.from_numpy(rgb).cuda()
    want_plain = denoise_ref.denoise(rgb, index, normal, point, albedo, **denoise_ref.DEFAULTS)
    before = dn.run(x, g)
    torch.cuda.synchronize()
    same_bits(before.cpu().numpy(), want_plain, "unguided run before")
    a, va = gpu_run(dn, rgb, var, g)
    b, vb = gpu_run(dn, rgb, var, g, in_place=True)
    same_bits(b, a, "in place")
    same_bits(vb, va, "in place (variance)")
    after = dn.run(x, g)
    torch.cuda.synchronize()
    same_bits(after.cpu().numpy(), want_plain, "unguided run after")
    c, vc = gpu_run(dn, rgb, var, g)
    same_bits(c, a, "guided run after an unguided one")
    same_bits(vc, va, "guided run after an unguided one (variance)")
    pack, lv = dn.timing()
    assert len(lv) == capi.DENOISE_GUIDED_DEFAULTS["levels"] and pack > 0 and all(0 < t < 1000 for t in lv)
    with pytest.raises(ValueError, match="var_rgb must be"):
        dn.run_guided(x, torch.zeros((h, w), device="cuda"), g)
    with pytest.raises(ValueError, match="unknown denoise parameter"):
        dn.run_guided(x, torch.zeros_like(x), g, sigma=1.0)
    with pytest.raises(capi.RayzHipError, match="var_floor"):
        dn.run_guided(x, torch.zeros_like(x), g, var_floor=0.0)
    dn.close()


def test_end_to_end_from_a_tracked_handle(gpu):
    """threeSpheres at 64x36: 16 spp in 8 passes on a tracked handle, `noise_rgb()` and `gbuffer()` feed `run_guided()` at its
    defaults.  The output is finite, equals the mirror fed the same downloads, and is nearer the 1024-spp frame than the noisy frame."""
    t = tracer.threeSpheres(64, seed=3)
    t.samples_per_px, t.max_bounces = 16, 8
    t.set_gpu(render_seed=17, chunk_spp=2, traversal=capi.TRAVERSAL_BVH, tmin=1e-3)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    ds = render.DeviceScene(sd)
    pr = ds.progressive(cam, p, track_noise=True)
    frame = torch.full((p.height, p.width, 3), float("nan"), device="cuda")
    torch.cuda.synchronize()
    passes = 0
    while not pr.done:
        pr.step(0, frame.data_ptr())
        passes += 1
    assert passes == 8 and pr.samples_done == 16
    var = pr.noise_rgb()
    pr.stats()
    g = ds.gbuffer(cam, p)
    ds.query_sync()
    dn = render.Denoiser(p.width, p.height)
    out, vout = dn.run_guided(frame, var, g, var_out=True)
    torch.cuda.synchronize()
    noisy, var_h, out_h, vout_h = (a.cpu().numpy() for a in (frame, var, out, vout))
    host = [getattr(g, k).cpu().numpy() for k in ("index", "normal", "point", "albedo")]
    assert np.isfinite(var_h).all() and (var_h >= 0).all() and (var_h > 0).any()
    assert np.isfinite(out_h).all() and np.isfinite(vout_h).all()
    want = denoise_guided_ref.denoise(noisy, var_h, *host, **capi.DENOISE_GUIDED_DEFAULTS)
    same_bits(out_h, want[0], "end to end")
    same_bits(vout_h, want[1], "end to end (variance)")
    p.samples_per_px, p.chunk_spp = 1024, 0
    ref = torch.empty_like(frame)
    torch.cuda.synchronize()
    ds.render_into(cam, p, ref.data_ptr())
    ds.sync()
    ref = ref.cpu().numpy().astype(np.float64)
    mse_noisy, mse_out = ((noisy - ref) ** 2).mean(), ((out_h - ref) ** 2).mean()
    print(f"threeSpheres 64x36, 16 spp: MSE against 1024 spp noisy {mse_noisy:.4e}, guided {mse_out:.4e}, ratio {mse_out / mse_noisy:.3f}")
    assert mse_out < mse_noisy, (mse_out, mse_noisy)
    pr.close()
    dn.close()
    ds.close()
