"""Guided upscaling on the GPU (rayz_hip_upscaler_*, `render.Upscaler`): colour, variance and stage map equal the CPU restatement of
DESIGN.md §4.20 (tests/upscale_mirror.cpp) bit for bit — the synthetic scenes of tests/upscale_scenes.py at sizes smaller than a
footprint, no multiple of a tile and across tile boundaries, for every factor, flag state, output set, normal power and form; the
hand cases of tests/upscale_cases.py against their rational answers directly; a rendered low-resolution frame under the library's
own G-buffers; repeatability, stream ordering, untouched inputs, and the refusals that need a live handle."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

import upscale_cases
import upscale_ref
import upscale_scenes
from rayz_amd import capi, render, tracer

pytestmark = pytest.mark.gpu

FORMS = (capi.UPSCALE_FORM_AUTO, capi.UPSCALE_FORM_DIRECT)  # every form this build has


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def assert_same(got, want, what):
    got, want = bits(got), bits(want)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ, first {bad[:4].tolist()}")


def to_gbuffer(g):
    r = render.QueryResult()
    r.index, r.normal, r.point = (torch.from_numpy(a).cuda() for a in (g.index, g.normal, g.point))
    r.albedo = torch.from_numpy(g.albedo).cuda() if g.albedo is not None else None
    return r


def gpu_run(up, rgb_lo, g_lo, g_hi, var_lo=None, stage=False, **prm):
    """One run on fresh copies of the inputs, which must come back unchanged.  Returns (out, var or None, stage or None) on the host."""
    host = [rgb_lo] + ([var_lo] if var_lo is not None else []) + [getattr(g, k) for g in (g_lo, g_hi) for k in ("index", "normal", "point", "albedo")
                                                                   if getattr(g, k) is not None]
    x = torch.from_numpy(rgb_lo).cuda()
    v = torch.from_numpy(var_lo).cuda() if var_lo is not None else None
    tl, th = to_gbuffer(g_lo), to_gbuffer(g_hi)
    prm.setdefault("flags", upscale_ref.ALBEDO)  # (the mirror's default; the library's is 0)
    res = up.run(x, tl, th, var_rgb=v, stage=stage, **prm)
    torch.cuda.synchronize()
    dev = [x] + ([v] if v is not None else []) + [getattr(g, k) for g in (tl, th) for k in ("index", "normal", "point", "albedo") if getattr(g, k) is not None]
    for a, b in zip(host, dev):
        assert np.array_equal(bits(a), bits(b.cpu().numpy())), "a run changed one of its inputs"
    res = list(res) if isinstance(res, tuple) else [res]
    out = res.pop(0).cpu().numpy()
    var = res.pop(0).cpu().numpy() if var_lo is not None else None
    stg = res.pop(0).cpu().numpy() if stage else None
    assert not res
    return out, var, stg


@pytest.mark.parametrize("w,h", upscale_scenes.SIZES)
def test_device_equals_the_mirror_on_the_synthetic_scenes(gpu, w, h):
    """factor x flag x normal power x (variance and stage map asked for or not); the form cycles."""
    form = itertools.cycle(FORMS)
    for f in upscale_scenes.FACTORS:
        s = upscale_scenes.synthetic_pair(w, h, f, seed=1)
        up = render.Upscaler(f * w, f * h, f)
        for flags, npl, extras in itertools.product((capi.DENOISE_ALBEDO, 0), (6, 0), (True, False)):
            prm = dict(flags=flags, normal_power_log2=npl, sigma_plane=0.3)
            var_lo = s["var_lo"] if extras else None
            want, want_var, want_stage = upscale_ref.upscale(s["rgb_lo"], s["g_lo"], s["g_hi"], f, var_rgb=var_lo, **prm)
            got, var, stage = gpu_run(up, s["rgb_lo"], s["g_lo"], s["g_hi"], var_lo=var_lo, stage=extras, form=next(form), **prm)
            what = f"{w}x{h} f={f} {prm} extras={extras}"
            assert_same(got, want, what + " colour")
            if extras:
                assert_same(var, want_var, what + " variance")
                assert np.array_equal(stage, want_stage), what + " stage map"
        up.close()


def test_every_form_gives_the_same_bits(gpu):
    w, h, f = 45, 23, 2
    s = upscale_scenes.synthetic_pair(w, h, f, seed=5)
    up = render.Upscaler(f * w, f * h, f)
    want = upscale_ref.upscale(s["rgb_lo"], s["g_lo"], s["g_hi"], f, var_rgb=s["var_lo"])
    assert set(np.unique(want[2]).tolist()) == {0, 1, 2}
    for form in FORMS:
        got = gpu_run(up, s["rgb_lo"], s["g_lo"], s["g_hi"], var_lo=s["var_lo"], stage=True, form=form)
        for a, b, name in zip(got, want, ("colour", "variance", "stage map")):
            assert_same(a, b, f"form {form} {name}")
    up.close()


def test_device_gives_the_rational_answers_bit_for_bit(gpu):
    """The hand cases against their closed-form answers directly, not through the mirror."""
    for c in upscale_cases.cases():
        H, W = c["labels_hi"].shape
        up = render.Upscaler(W, H, c["f"])
        out, var, stage = gpu_run(up, c["rgb_lo"], c["g_lo"], c["g_hi"], var_lo=c.get("var_lo"), stage=True)
        want, want_var, want_stage = upscale_cases.expected(c)
        m = c.get("check", np.ones((H, W), bool))
        assert np.array_equal(stage[m], want_stage[m]), c["name"]
        assert np.array_equal(bits(out)[m], bits(want)[m]), c["name"]
        if want_var is not None:
            assert np.array_equal(bits(var)[m], bits(want_var)[m]), c["name"]
        up.close()


def _three_spheres():
    t = tracer.threeSpheres(96, seed=3)
    t.samples_per_px, t.max_bounces = 4, 8
    t.set_gpu(render_seed=17, chunk_spp=4)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    p.traversal, p.tmin = capi.TRAVERSAL_BVH, 1e-3
    return sd, cam, p


def _host_guides(g):
    return upscale_ref.Guides(*(getattr(g, k).cpu().numpy() for k in ("index", "normal", "point", "albedo")))


def test_a_rendered_pair(gpu):
    """The three-spheres scene: a 4-spp frame at 48x27 under the library's own G-buffers at 48x27 and 96x54, the low-resolution
    camera being `lowres_camera`'s; and, on the caller's stream with no synchronisation in between, the render of that frame and the
    run that reads it."""
    sd, cam, p = _three_spheres()
    f = 2
    cam_lo, p_lo = render.lowres_camera(cam, f), render.lowres_params(p, f)
    assert (p.width, p.height, p_lo.width, p_lo.height) == (96, 54, 48, 27)
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
    assert len(np.unique(h_lo.index)) >= 3 and len(np.unique(h_hi.index)) >= 3  # the ground and at least two balls
    rgb = frame.cpu().numpy()
    var_lo = torch.full((27, 48, 3), 0.01, dtype=torch.float32, device="cuda") * (frame + 0.1)
    up = render.Upscaler(96, 54, f)
    for prm in (dict(flags=capi.DENOISE_ALBEDO), dict(flags=0, normal_power_log2=0, sigma_plane=0.1)):
        want, want_var, want_stage = upscale_ref.upscale(rgb, h_lo, h_hi, f, var_rgb=var_lo.cpu().numpy(), **{**upscale_ref.DEFAULTS, **prm})
        out, var, stage = up.run(frame, g_lo, g_hi, var_rgb=var_lo, stage=True, **prm)
        torch.cuda.synchronize()
        assert_same(out.cpu().numpy(), want, f"rendered pair {prm} colour")
        assert_same(var.cpu().numpy(), want_var, f"rendered pair {prm} variance")
        assert np.array_equal(stage.cpu().numpy(), want_stage)
        assert np.isfinite(want).all() and (want_stage == 0).mean() > 0.5
    # the caller's stream: render, then upscale, nothing in between
    s = torch.cuda.Stream()
    frame2 = torch.full((27, 48, 3), float("nan"), device="cuda")
    torch.cuda.synchronize()
    ds.render_into(cam_lo, p_lo, frame2.data_ptr(), stream=s.cuda_stream)
    out2 = up.run(frame2, g_lo, g_hi, stream=s.cuda_stream)
    s.synchronize()
    ds.sync()
    assert_same(frame2.cpu().numpy(), rgb, "the same frame twice")
    assert_same(out2.cpu().numpy(), upscale_ref.upscale(rgb, h_lo, h_hi, f, flags=capi.UPSCALE_DEFAULTS["flags"])[0], "run ordered after a render on the caller's stream")
    up.close()
    ds.close()


def test_two_runs_on_one_handle_timing_and_the_checks_behind_the_handle(gpu):
    w, h, f = 33, 17, 3
    s = upscale_scenes.synthetic_pair(w, h, f, seed=7)
    up = render.Upscaler(f * w, f * h, f)
    with pytest.raises(capi.RayzHipError, match="no upscaler run"):
        up.timing()
    a = gpu_run(up, s["rgb_lo"], s["g_lo"], s["g_hi"], var_lo=s["var_lo"], stage=True)
    other = gpu_run(up, s["rgb_lo"][::-1].copy(), s["g_lo"], s["g_hi"], flags=0)  # a different run in between leaves nothing behind
    b = gpu_run(up, s["rgb_lo"], s["g_lo"], s["g_hi"], var_lo=s["var_lo"], stage=True)
    for x, y, name in zip(a, b, ("colour", "variance", "stage map")):
        assert_same(y, x, f"second run on one handle: {name}")
    assert not np.array_equal(other[0], a[0])
    pack, rec = up.timing()
    assert 0 < pack < 1000 and 0 < rec < 1000
    # refused behind the handle: another factor than the handle's; an output overlapping an input without starting where it starts
    lib = capi.load()
    x = torch.from_numpy(s["rgb_lo"]).cuda()
    tl, th = to_gbuffer(s["g_lo"]), to_gbuffer(s["g_hi"])
    need = ("index", "normal", "point", "albedo")
    ol, oh = render._gbuffer_pointers(tl, need), render._gbuffer_pointers(th, need)
    out = torch.empty((f * h, f * w, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()

    def rc(factor, out_ptr):
        prm = capi.UpscaleParams(factor=factor, **capi.UPSCALE_DEFAULTS)
        return lib.rayz_hip_upscaler_run(up._h, C.byref(prm), C.c_void_p(x.data_ptr()), None, C.byref(ol), C.byref(oh), C.c_void_p(out_ptr), None, None, None)

    assert rc(2, out.data_ptr()) == capi.ERR_BAD_ARG and b"handle was created for 3" in lib.rayz_hip_last_error()
    assert rc(3, th.normal.data_ptr() + 12) == capi.ERR_BAD_ARG and b"aliases" in lib.rayz_hip_last_error()
    assert rc(3, out.data_ptr()) == capi.OK
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy(), upscale_ref.upscale(s["rgb_lo"], s["g_lo"], s["g_hi"], f, flags=capi.UPSCALE_DEFAULTS["flags"])[0], "through the C ABI")
    with pytest.raises(ValueError, match="must be"):
        up.run(x[:, :-1].contiguous(), tl, th)
    with pytest.raises(ValueError, match="unknown upscale parameter"):
        up.run(x, tl, th, factor=2)
    with pytest.raises(ValueError, match="var_out needs var_rgb"):
        up.run(x, tl, th, var_out=out)
    up.close()
