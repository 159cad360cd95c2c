"""Guided upscaling with a phase on the GPU (rayz_hip_upscaler_run_phase, `Upscaler.run(..., phase=)`; DESIGN.md §4.20 "Lattice
samples"): colour, variance and stage map equal tests/upscale_phase_mirror.cpp bit for bit on lattices of the synthetic scenes,
the hand cases come out at their rational answers, and a rendered lattice frame passes through at its own pixels."""
import numpy as np
import pytest
import torch

import upscale_phase_cases as cases
import upscale_scenes
from rayz_amd import capi, render, tracer
from test_upscale_gpu import assert_same, bits, to_gbuffer

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (2, 1), (1, 3), (4, 3), (9, 5)]  # low-resolution (w, h)


def gpu_run(up, rgb_lo, g_lo, g_hi, phase, var_lo=None, **prm):
    x = torch.from_numpy(rgb_lo).cuda()
    v = torch.from_numpy(var_lo).cuda() if var_lo is not None else None
    res = up.run(x, to_gbuffer(g_lo), to_gbuffer(g_hi), var_rgb=v, stage=True, phase=phase, **prm)
    torch.cuda.synchronize()
    res = [t.cpu().numpy() for t in res]
    return (res[0], res[1], res[2]) if v is not None else (res[0], None, res[1])


@pytest.mark.parametrize("f", upscale_scenes.FACTORS)
@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_the_phase_mirror(gpu, w, h, f):
    """Every phase on the diagonal and one off it, both flag states; with and without the variance."""
    s = upscale_scenes.synthetic_pair(w, h, f, seed=1)
    up = render.Upscaler(f * w, f * h, f)
    stages = set()
    for k, phase in enumerate([(d, d) for d in range(f)] + [(f - 1, 0)]):
        g_lo = cases.lattice(s["g_hi"], f, phase)
        for flags in (capi.DENOISE_ALBEDO, 0):
            var_lo = s["var_lo"] if (k + flags) % 2 == 0 or phase[0] != phase[1] else None
            prm = dict(flags=flags, sigma_plane=0.3)
            want, want_var, want_stage = cases.upscale(s["rgb_lo"], g_lo, s["g_hi"], f, phase, var_rgb=var_lo, **prm)
            got, var, stage = gpu_run(up, s["rgb_lo"], g_lo, s["g_hi"], phase, var_lo=var_lo, **prm)
            what = f"{w}x{h} f={f} phase={phase} flags={flags}"
            assert_same(got, want, what + " colour")
            assert np.array_equal(stage, want_stage), what + " stage map"
            if var_lo is not None:
                assert_same(var, want_var, what + " variance")
            stages |= set(np.unique(stage).tolist())
            # the samples pass through: the raw colour at every sampled pixel (its own guides accept it)
            assert_same(got[phase[1]::f, phase[0]::f], s["rgb_lo"], what + " samples")
    if (w, h) == SIZES[-1]:
        assert stages == {0, 1, 2}
    up.close()


def test_device_gives_the_rational_answers_bit_for_bit(gpu):
    for c in cases.cases():
        H, W = c["labels_hi"].shape
        up = render.Upscaler(W, H, c["f"])
        out, var, stage = gpu_run(up, c["rgb_lo"], c["g_lo"], c["g_hi"], c["phase"], var_lo=c.get("var_lo"), flags=c.get("flags", 1))
        want, want_var, want_stage = cases.expected(c)
        m = c.get("check", np.ones((H, W), bool))
        assert np.array_equal(stage[m], want_stage[m]), c["name"]
        assert np.array_equal(bits(out)[m], bits(want)[m]), c["name"]
        if want_var is not None:
            assert np.array_equal(bits(var)[m], bits(want_var)[m]), c["name"]
        up.close()


def test_the_run_without_a_phase_is_untouched_and_a_bad_phase_is_refused(gpu):
    w, h, f = 9, 5, 3
    s = upscale_scenes.synthetic_pair(w, h, f, seed=3)
    up = render.Upscaler(f * w, f * h, f)
    x, tl, th = torch.from_numpy(s["rgb_lo"]).cuda(), to_gbuffer(s["g_lo"]), to_gbuffer(s["g_hi"])
    import upscale_ref

    plain = up.run(x, tl, th, flags=capi.DENOISE_ALBEDO)
    torch.cuda.synchronize()
    assert_same(plain.cpu().numpy(), upscale_ref.upscale(s["rgb_lo"], s["g_lo"], s["g_hi"], f)[0], "phase=None is the run of block means")
    for bad in ((3, 0), (0, 3), (-1, 0)):
        with pytest.raises(ValueError, match="phase"):
            up.run(x, tl, th, phase=bad)
    up.close()


@pytest.mark.parametrize("f", [2, 3, 4])
def test_a_rendered_lattice_passes_through_at_its_own_pixels(gpu, f):
    """A 24x24 frame of the three-spheres scene: the lattice frame of a phase, traced as a sparse render, under gbuffer_lo =
    gbuffer_hi.lattice(...): the output at the lattice's pixels is the lattice frame's bits (and so the whole frame's)."""
    t = tracer.threeSpheres(24, seed=3)
    t.samples_per_px, t.max_bounces = 8, 4
    t.set_gpu(render_seed=17, chunk_spp=4)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    p.height, p.tmin = 24, 1e-3
    ds = render.DeviceScene(sd)
    frame = torch.empty((24, 24, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ds.render_into(cam, p, frame.data_ptr())
    ds.sync()
    g_hi = ds.gbuffer(cam, p)
    ds.query_sync()
    up = render.Upscaler(24, 24, f)
    n = 24 // f
    for phase in ((0, 0), (f - 1, 1)):
        pixels, dest = render.lattice_pixels(24, 24, f, phase, device="cuda")
        lo = torch.empty((n, n, 3), dtype=torch.float32, device="cuda")
        var = torch.empty((n, n, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ds.render_pixels(cam, p, pixels, dest=dest, out=lo, var=var)
        ds.sync()
        g_lo = g_hi.lattice(f, phase)
        for flags in (capi.DENOISE_ALBEDO, 0):
            out, var_out, stage = up.run(lo, g_lo, g_hi, var_rgb=var, stage=True, phase=phase, flags=flags)
            torch.cuda.synchronize()
            px, py = phase
            assert torch.equal(out[py::f, px::f].view(torch.int32), lo.view(torch.int32)), (f, phase, flags)
            assert torch.equal(out[py::f, px::f].view(torch.int32), frame[py::f, px::f].contiguous().view(torch.int32))
            assert torch.equal(var_out[py::f, px::f], var.clamp(0.0, 4294967296.0)) and (stage[py::f, px::f] == 0).all()
            assert torch.isfinite(out).all()
    up.close()
    ds.close()
