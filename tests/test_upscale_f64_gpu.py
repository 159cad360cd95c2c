"""Guided upscaling on the GPU against the float64 statement of DESIGN.md §4.20 (tests/upscale_f64.py) DIRECTLY: the colour and the
variance of `Upscaler.run(...)` and of `Upscaler.run(..., phase=...)` stay within the reference's derived per-value bounds at every
pixel it does not exclude, the values it calls selections are equal, and the stage map is equal.  The comparison is redundant with
"device == mirror" (tests/test_upscale_gpu.py, tests/test_upscale_phase_gpu.py) and "mirror within the bound"
(tests/test_upscale_f64_cpu.py) by design: it survives an edit of the mirrors.

Frames: low-resolution 17x9 and 45x23 under f = 2, 3, 4 — full frames from 34x18 to 180x92, no multiple of the 32x8 tile on either
axis, up to six tiles across and twelve down, which takes the phase kernel across tile borders too — of `synthetic_pair` and of
`curved_pair`, whose guide weights are not 0 or 1; and a rendered pair and a rendered lattice under the library's own G-buffers."""
import numpy as np
import pytest
import torch

import upscale_f64 as u64
from rayz_amd import capi, render, tracer
from test_upscale_f64_cpu import EXCLUDED_CAP, FACTORS, SCENES, SIGMA_PLANE, kinds, pair, ratios, reference
from test_upscale_gpu import _host_guides, _three_spheres, to_gbuffer

pytestmark = pytest.mark.gpu

A = capi.DENOISE_ALBEDO
SIZES = ((17, 9), (45, 23))  # low-resolution (w, h)
# (flags, normal_power_log2, variance and stage map asked for): the two sets alternate over (factor, run kind), so that both flag
# states meet both powers, and both instantiations of each kernel run, on block means and with a phase, at every size
STATES = (((A, 6, True), (0, 0, False)), ((A, 0, False), (0, 6, True)))


def within(got, ref, what):
    """The device's (colour, variance or None, stage map or None) against the reference with its bounds: the exclusion cap, then
    every kept value within its bound and the stage map equal.  Prints the worst |err| / bound."""
    excluded = ref[5]
    print(f"device vs f64: {what}: excluded {int(excluded.sum())} of {excluded.size}")
    assert excluded.mean() <= EXCLUDED_CAP, (what, int(excluded.sum()))
    assert np.isfinite(got[0]).all() and (got[1] is None or np.isfinite(got[1]).all()), what
    rc, rv, ns = ratios((got[0], got[1], ref[4] if got[2] is None else got[2]), *ref)
    print(f"device vs f64: {what}: max err/bound colour {rc:.4f}" + (f", variance {rv:.4f}" if got[1] is not None else ""))
    assert ns == 0, (what, "stage map", ns)
    assert rc <= 1 and rv <= 1, (what, rc, rv)
    return rc, rv


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("scene", SCENES)
def test_device_is_within_the_bound_of_the_f64_reference(gpu, scene, w, h):
    """Both runs, three phases, f = 2, 3, 4, four parameter states; one handle per factor, built, run and closed here."""
    worst = {"block means": [0.0, 0.0], "phase": [0.0, 0.0]}
    for fi, f in enumerate(FACTORS):
        up = render.Upscaler(f * w, f * h, f)
        try:
            for ki, phase in enumerate(kinds(f)):
                s = pair(scene, w, h, f, phase)
                x, v = torch.from_numpy(s["rgb_lo"]).cuda(), torch.from_numpy(s["var_lo"]).cuda()
                tl, th = to_gbuffer(s["g_lo"]), to_gbuffer(s["g_hi"])
                for flags, npl, extras in STATES[(fi + ki) % 2]:
                    res = up.run(x, tl, th, var_rgb=v if extras else None, stage=extras, phase=phase, flags=flags, normal_power_log2=npl,
                                 sigma_plane=SIGMA_PLANE)
                    torch.cuda.synchronize()
                    got = [t.cpu().numpy() for t in res] if extras else [res.cpu().numpy(), None, None]
                    ref = reference(s, f, phase, flags, npl, extras, bound=True)
                    rc, rv = within(got, ref, f"{scene} {w}x{h} f={f} phase={phase} flags={flags} k={npl} extras={extras}")
                    k = worst["block means" if phase is None else "phase"]
                    k[0], k[1] = max(k[0], rc), max(k[1], rv)
        finally:
            up.close()
    for kind, (rc, rv) in worst.items():
        print(f"device vs f64, {scene} {w}x{h}, {kind}: worst err/bound colour {rc:.4f}, variance {rv:.4f}")


def test_a_rendered_pair_and_a_rendered_lattice(gpu):
    """The three-spheres scene under the library's own G-buffers, the reference fed the device's arrays: a 4-spp frame at 48x27 from
    `lowres_camera` under 96x54 (the setup of tests/test_upscale_gpu.py's rendered pair), and a lattice frame of a 24x24 frame at
    f = 2, traced as a sparse render, under `gbuffer.lattice`."""
    sd, cam, p = _three_spheres()
    f = 2
    cam_lo, p_lo = render.lowres_camera(cam, f), render.lowres_params(p, f)
    ds = render.DeviceScene(sd)
    frame = torch.empty((27, 48, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ds.render_into(cam_lo, p_lo, frame.data_ptr())
    ds.sync()
    g_lo = ds.gbuffer(cam_lo, p_lo)
    ds.query_sync()
    g_hi = ds.gbuffer(cam, p)
    ds.query_sync()
    h_lo, h_hi = _host_guides(g_lo), _host_guides(g_hi)
    var_lo = torch.full((27, 48, 3), 0.01, dtype=torch.float32, device="cuda") * (frame + 0.1)
    rgb, var = frame.cpu().numpy(), var_lo.cpu().numpy()
    up = render.Upscaler(96, 54, f)
    try:
        for prm in (dict(flags=A, normal_power_log2=6, sigma_plane=0.25), dict(flags=0, normal_power_log2=0, sigma_plane=0.1)):
            res = up.run(frame, g_lo, g_hi, var_rgb=var_lo, stage=True, **prm)
            torch.cuda.synchronize()
            ref = u64.upscale_f64(rgb, h_lo, h_hi, f, var, bound=True, **prm)
            within([t.cpu().numpy() for t in res], ref, f"rendered pair 48x27 f=2 {prm}")
            d = {}
            u64.upscale_f64(rgb, h_lo, h_hi, f, var, detail=d, **prm)
            g = d["g0"][d["accepted0"]]
            share = float(((g > 0.01) & (g < 0.99)).mean())
            print(f"rendered pair {prm}: share of accepted stage-0 taps with 0.01 < g < 0.99: {share:.3f}")
            assert share > 0  # (curved surfaces: weights that are not 0 or 1)
    finally:
        up.close()
        ds.close()
    # the lattice: a 24x24 frame, every second pixel traced
    t = tracer.threeSpheres(24, seed=3)
    t.samples_per_px, t.max_bounces = 8, 4
    t.set_gpu(render_seed=17, chunk_spp=4)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    p.height, p.tmin = 24, 1e-3
    ds = render.DeviceScene(sd)
    g_hi = ds.gbuffer(cam, p)
    ds.query_sync()
    h_hi = _host_guides(g_hi)
    up = render.Upscaler(24, 24, f)
    try:
        for phase in ((0, 0), (1, 0)):
            pixels, dest = render.lattice_pixels(24, 24, f, phase, device="cuda")
            lo = torch.empty((12, 12, 3), dtype=torch.float32, device="cuda")
            lo_var = torch.empty((12, 12, 3), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ds.render_pixels(cam, p, pixels, dest=dest, out=lo, var=lo_var)
            ds.sync()
            g_lo = g_hi.lattice(f, phase)
            h_lo = _host_guides(g_lo)
            for flags in (A, 0):
                prm = dict(flags=flags, normal_power_log2=6, sigma_plane=0.25)
                res = up.run(lo, g_lo, g_hi, var_rgb=lo_var, stage=True, phase=phase, **prm)
                torch.cuda.synchronize()
                ref = u64.upscale_f64(lo.cpu().numpy(), h_lo, h_hi, f, lo_var.cpu().numpy(), phase, bound=True, **prm)
                within([t.cpu().numpy() for t in res], ref, f"rendered lattice 12x12 f=2 phase={phase} flags={flags}")
    finally:
        up.close()
        ds.close()
