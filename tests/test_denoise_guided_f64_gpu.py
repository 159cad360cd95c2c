"""The variance-guided denoiser on the GPU against the float64 statement of DESIGN.md §4.13 (tests/denoise_guided_f64.py) DIRECTLY:
`Denoiser.run_guided`'s colour and variance output stay within the reference's derived per-value bounds at every pixel it does not
exclude — at 1, 2, 5 and 8 levels with and without demodulation, with every level read from global memory and with the levels up
to stride 4 staged in LDS, at the tap of `run_guided(tap_level=)`, and on a rendered frame.  The comparison is redundant with
"device == mirror" (tests/test_denoise_guided_gpu.py) and "mirror within the bound" (tests/test_denoise_guided_f64_cpu.py) by
design: it survives an edit of the mirror.

Frames: 63x65 and 131x77 — no multiple of the 32x8 tile on either axis, the second more than four tiles across, each with a dimension
below the stride 2^7 of the eighth level and with pixels nearer the border than every halo."""
import functools

import numpy as np
import pytest
import torch

import denoise_guided_f64 as g64
from denoise_cases import synthetic
from denoise_guided_cases import guided_variance
from rayz_amd import capi, render, tracer

pytestmark = pytest.mark.gpu

FRAMES = ((63, 65, 6365, 7), (131, 77, 5, 11))  # (width, height, seed of synthetic(), seed of guided_variance())
LEVELS = (1, 2, 5, 8)
PRM = dict(sigma_color=2.0, sigma_plane=0.3, var_floor=1e-4, normal_power_log2=6)
EXCLUDED_CAP = 0.001


@functools.lru_cache(maxsize=None)
def inputs(frame):
    w, h, seed, vseed = FRAMES[frame]
    rgb, index, normal, point, albedo = synthetic(w, h, seed)
    return rgb, guided_variance(rgb, vseed), index, normal, point, albedo


@functools.lru_cache(maxsize=None)
def reference(frame, flags):
    """{L: (colour, colour bound, variance, variance bound, excluded)} for LEVELS: computed once, shared, never changed."""
    return g64.denoise_guided_f64(*inputs(frame), levels=8, want_levels=LEVELS, bound=True, flags=flags, **PRM)


def to_gbuffer(index, normal, point, albedo):
    g = render.QueryResult()
    g.index, g.normal, g.point, g.albedo = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (index, normal, point, albedo))
    return g


def within(got, ref, what, var=True):
    """The device's colour (and variance) against one level of the reference: the exclusion cap, then every kept value within its
    bound.  Prints the worst |err| / bound."""
    out, cb, vout, vb, excluded = ref
    assert excluded.mean() <= EXCLUDED_CAP, (what, int(excluded.sum()))
    keep = ~excluded
    assert np.isfinite(got[0]).all(), what
    rc = float((np.abs(got[0].astype(np.float64) - out)[keep] / cb[keep]).max())
    rv = 0.0
    if var:
        assert np.isfinite(got[1]).all(), what
        rv = float((np.abs(got[1].astype(np.float64) - vout)[keep] / vb[keep]).max())
    print(f"device vs f64: {what}: max err/bound colour {rc:.4f}" + (f", variance {rv:.4f}" if var else "") + f", excluded {int(excluded.sum())}")
    assert rc <= 1 and rv <= 1, (what, rc, rv)


def run_frames(staging, what):
    """Both frames, both flag states, LEVELS: one handle per frame, built, run and closed here."""
    for frame, (w, h, _, _) in enumerate(FRAMES):
        rgb, var, index, normal, point, albedo = inputs(frame)
        g = to_gbuffer(index, normal, point, albedo)
        x, v = torch.from_numpy(rgb).cuda(), torch.from_numpy(var).cuda()
        dn = render.Denoiser(w, h)
        try:
            for flags in (capi.DENOISE_ALBEDO, 0):
                ref = reference(frame, flags)
                for L in LEVELS:
                    render.debug_set(capi.DEBUG_DENOISE_LDS_STRIDE, staging)
                    try:
                        out, vout = dn.run_guided(x, v, g, var_out=True, levels=L, flags=flags, **PRM)
                    finally:
                        render.debug_set(capi.DEBUG_DENOISE_LDS_STRIDE, -1)
                    torch.cuda.synchronize()
                    within((out.cpu().numpy(), vout.cpu().numpy()), ref[L], f"{what} {w}x{h} L={L} flags={flags}")
        finally:
            dn.close()


def test_run_guided_is_within_the_bound_of_the_f64_reference(gpu):
    """synthetic() guides, guided_variance() variances, the built-in choice of each level's form."""
    run_frames(-1, "built-in staging")


@pytest.mark.parametrize("staging", (0, 4))
def test_both_level_forms_are_within_the_bound(gpu, staging):
    """RAYZ_DEBUG_DENOISE_LDS_STRIDE 0: every level reads its taps from global memory; 4: the levels of stride 1, 2 and 4 are staged
    in LDS — with the test above every level has run in each form it has."""
    run_frames(staging, f"staging={staging}")


def test_the_tap_is_within_the_bound_of_its_level(gpu):
    """`run_guided(levels=5, tap_level=t)`, t = 1 and 2: the tapped colour against the reference's level-t colour, the final colour
    and variance against level 5."""
    for frame, (w, h, _, _) in enumerate(FRAMES):
        rgb, var, index, normal, point, albedo = inputs(frame)
        g = to_gbuffer(index, normal, point, albedo)
        x, v = torch.from_numpy(rgb).cuda(), torch.from_numpy(var).cuda()
        ref = reference(frame, capi.DENOISE_ALBEDO)
        dn = render.Denoiser(w, h)
        try:
            for t in (1, 2):
                out, vout, tap = dn.run_guided(x, v, g, var_out=True, levels=5, tap_level=t, flags=capi.DENOISE_ALBEDO, **PRM)
                torch.cuda.synchronize()
                within((tap.cpu().numpy(), None), ref[t], f"tap {w}x{h} tap_level={t}", var=False)
                within((out.cpu().numpy(), vout.cpu().numpy()), ref[5], f"tapped run {w}x{h} tap_level={t} L=5")
        finally:
            dn.close()


def test_a_rendered_frame_is_within_the_bound(gpu):
    """The end-to-end test's own setup: threeSpheres at 64x36, 16 spp in 8 passes on a tracked handle, `noise_rgb()` and `gbuffer()`
    feeding `run_guided()` at its defaults; the reference is fed the same device arrays.  A rendered scene has grazing pixels the
    synthetic guides lack, so the count of excluded pixels is printed before the 0.1 % cap is applied."""
    t = tracer.threeSpheres(64, seed=3)
    t.samples_per_px, t.max_bounces = 16, 8
    t.set_gpu(render_seed=17, chunk_spp=2, traversal=capi.TRAVERSAL_BVH, tmin=1e-3)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    ds = render.DeviceScene(sd)
    pr = ds.progressive(cam, p, track_noise=True)
    dn = render.Denoiser(p.width, p.height)
    try:
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
        out, vout = dn.run_guided(frame, var, g, var_out=True)
        torch.cuda.synchronize()
        noisy, var_h, out_h, vout_h = (a.cpu().numpy() for a in (frame, var, out, vout))
        host = [getattr(g, k).cpu().numpy() for k in ("index", "normal", "point", "albedo")]
    finally:
        pr.close()
        dn.close()
        ds.close()
    L = capi.DENOISE_GUIDED_DEFAULTS["levels"]
    ref = g64.denoise_guided_f64(noisy, var_h, *host, bound=True, **capi.DENOISE_GUIDED_DEFAULTS)[L]
    print(f"threeSpheres {p.width}x{p.height}: {int(ref[4].sum())} of {ref[4].size} pixels excluded, {int((host[0] < 0).sum())} background")
    within((out_h, vout_h), ref, f"threeSpheres {p.width}x{p.height} L={L}")
