"""The footprint albedo on the GPU (rayz_hip_upscaler_footprint_albedo, `render.Upscaler.footprint_albedo`, `run(footprint=True)`;
DESIGN.md §4.24): albedo and count equal the CPU restatement (tests/footprint_mirror.cpp) bit for bit on the scenes of
tests/footprint_scenes.py — a single pixel, less than a tile, across the 32x8 tile and the 64-lane boundary in both directions, every
factor, with and without the count —; the hand cases against their answers directly; the composed run against the upscale mirror fed
the mirror's filtered albedo; the capability itself (irradiance x full-size albedo, exactly); the handle's ordering, timing and
refusals; the defaults; a rendered pair under the library's own G-buffers."""
import ctypes as C

import numpy as np
import pytest
import torch

import footprint_cases
import footprint_ref
import footprint_scenes
import upscale_ref
from rayz_amd import capi, render, tracer

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def assert_same(got, want, what):
    got, want = bits(got), bits(want)
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} values differ, first {bad[:4].tolist()}")


def to_gbuffer(g, keys=("index", "normal", "point", "albedo")):
    r = render.QueryResult()
    for k in keys:
        setattr(r, k, torch.from_numpy(np.array(getattr(g, k))).cuda())
    return r


def gpu_footprint(up, g_lo, g_hi, count):
    """One call on fresh copies of index and albedo alone (nothing else is required), which must come back unchanged.  Returns
    (albedo, count or None) on the host."""
    tl, th = to_gbuffer(g_lo, ("index", "albedo")), to_gbuffer(g_hi, ("index", "albedo"))
    res = up.footprint_albedo(tl, th, count=count)
    torch.cuda.synchronize()
    for g, t in ((g_lo, tl), (g_hi, th)):
        for k in ("index", "albedo"):
            assert np.array_equal(bits(getattr(g, k)), bits(getattr(t, k).cpu().numpy())), "the call changed one of its inputs"
    if count:
        return res[0].cpu().numpy(), res[1].cpu().numpy()
    return res.cpu().numpy(), None


@pytest.mark.parametrize("w,h", footprint_scenes.SIZES)
def test_device_equals_the_mirror(gpu, w, h):
    for f in footprint_scenes.FACTORS:
        s = footprint_scenes.pair(w, h, f, 1)
        want, want_count = footprint_ref.footprint_guides(s["g_lo"], s["g_hi"], f)
        up = render.Upscaler(f * w, f * h, f)
        for count in (True, False):
            got, n = gpu_footprint(up, s["g_lo"], s["g_hi"], count)
            assert_same(got, want, f"{w}x{h} f={f} count={count} albedo")
            if count:
                assert np.array_equal(n, want_count), f"{w}x{h} f={f} count"
        up.close()


def test_device_gives_the_hand_answers(gpu):
    """The hand cases against their answers directly, not through the mirror."""
    for c in footprint_cases.cases():
        h, w = c["index_lo"].shape
        f = c["f"]
        up = render.Upscaler(f * w, f * h, f)
        tl, th = render.QueryResult(), render.QueryResult()
        tl.index, tl.albedo = torch.from_numpy(c["index_lo"]).cuda(), torch.from_numpy(c["albedo_lo"]).cuda()
        th.index, th.albedo = torch.from_numpy(c["index_hi"]).cuda(), torch.from_numpy(c["albedo_hi"]).cuda()
        out, n = up.footprint_albedo(tl, th, count=True)
        torch.cuda.synchronize()
        assert np.array_equal(n.cpu().numpy(), c["want_count"]), c["name"]
        assert_same(out.cpu().numpy(), c["want"], c["name"])
        up.close()


@pytest.mark.parametrize("f", (2, 4))
def test_the_composed_run_equals_the_upscale_mirror_on_the_filtered_albedo(gpu, f):
    w, h = 17, 9
    s = footprint_scenes.pair(w, h, f, 1)
    filtered, _ = footprint_ref.footprint_guides(s["g_lo"], s["g_hi"], f)
    g = upscale_ref.Guides(s["g_lo"].index, s["g_lo"].normal, s["g_lo"].point, filtered)
    want = upscale_ref.upscale(s["rgb_lo"], g, s["g_hi"], f, var_rgb=s["var_lo"], flags=upscale_ref.ALBEDO)
    assert set(np.unique(want[2]).tolist()) == {0, 1, 2}
    up = render.Upscaler(f * w, f * h, f)
    x, v = torch.from_numpy(s["rgb_lo"].copy()).cuda(), torch.from_numpy(s["var_lo"].copy()).cuda()
    tl, th = to_gbuffer(s["g_lo"]), to_gbuffer(s["g_hi"])
    given = tl.albedo
    out, var, stage = up.run(x, tl, th, var_rgb=v, stage=True, footprint=True, flags=capi.DENOISE_ALBEDO)
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy(), want[0], f"f={f} colour")
    assert_same(var.cpu().numpy(), want[1], f"f={f} variance")
    assert np.array_equal(stage.cpu().numpy(), want[2])
    assert tl.albedo is given and np.array_equal(bits(tl.albedo.cpu().numpy()), bits(s["g_lo"].albedo))  # the caller's G-buffer is as it was
    # .. and it is not what the point-sampled albedo gives
    plain = upscale_ref.upscale(s["rgb_lo"], s["g_lo"], s["g_hi"], f, var_rgb=s["var_lo"], flags=upscale_ref.ALBEDO)[0]
    assert not np.array_equal(bits(plain), bits(want[0]))
    up.close()


def test_the_capability_on_the_device(gpu):
    """★ The one-pixel checker under E = (2, 1, 1/2): run(footprint=True) returns E x albedo_hi exactly; the run as it was is off by
    the factor 2 in the channels the checker varies in."""
    c = footprint_cases.capability_case()
    f, a_hi = c["f"], c["albedo_hi"]
    H, W = a_hi.shape[:2]
    truth = c["E"] * a_hi
    up = render.Upscaler(W, H, f)
    x = torch.from_numpy(c["rgb_lo"]).cuda()
    tl, th = to_gbuffer(c["g_lo"](c["point_A"])), to_gbuffer(c["g_hi"])
    out, stage = up.run(x, tl, th, stage=True, footprint=True, flags=capi.DENOISE_ALBEDO)
    torch.cuda.synchronize()
    assert (stage.cpu().numpy() == 0).all()
    assert_same(out.cpu().numpy(), truth, "E x albedo_hi")
    flawed = up.run(x, tl, th, flags=capi.DENOISE_ALBEDO)
    torch.cuda.synchronize()
    assert_same(flawed.cpu().numpy()[..., 0], 2 * truth[..., 0], "the point sample's factor 2")
    up.close()


def test_handle_ordering_timing_and_refusals(gpu):
    w, h, f = 33, 9, 3
    s = footprint_scenes.pair(w, h, f, 1)
    lib = capi.load()
    up = render.Upscaler(f * w, f * h, f)
    ms = C.c_float(-1.0)
    assert lib.rayz_hip_upscaler_footprint_timing(up._h, C.byref(ms)) == capi.ERR_STATE and b"footprint" in lib.rayz_hip_last_error()
    with pytest.raises(capi.RayzHipError):
        up.footprint_timing()
    want, want_count = footprint_ref.footprint_guides(s["g_lo"], s["g_hi"], f)
    a = gpu_footprint(up, s["g_lo"], s["g_hi"], True)
    b = gpu_footprint(up, s["g_lo"], s["g_hi"], True)  # repeatable
    for got in (a, b):
        assert_same(got[0], want, "albedo")
        assert np.array_equal(got[1], want_count)
    assert 0 < up.footprint_timing() < 1000
    with pytest.raises(capi.RayzHipError, match="no upscaler run"):  # a footprint call is no run
        up.timing()
    # a run, a footprint call and a run on one handle, on the caller's stream with nothing in between; the second run reads what
    # the footprint call wrote
    x, v = torch.from_numpy(s["rgb_lo"].copy()).cuda(), torch.from_numpy(s["var_lo"].copy()).cuda()
    tl, th = to_gbuffer(s["g_lo"]), to_gbuffer(s["g_hi"])
    tf = to_gbuffer(s["g_lo"], ("index", "normal", "point"))
    st = torch.cuda.Stream()
    torch.cuda.synchronize()
    out1 = up.run(x, tl, th, stream=st.cuda_stream, flags=capi.DENOISE_ALBEDO)
    filtered = up.footprint_albedo(tl, th, stream=st.cuda_stream)
    tf.albedo = filtered
    out2 = up.run(x, tf, th, stream=st.cuda_stream, flags=capi.DENOISE_ALBEDO)
    st.synchronize()
    g = upscale_ref.Guides(s["g_lo"].index, s["g_lo"].normal, s["g_lo"].point, want)
    assert_same(out1.cpu().numpy(), upscale_ref.upscale(s["rgb_lo"], s["g_lo"], s["g_hi"], f, flags=upscale_ref.ALBEDO)[0], "run before")
    assert_same(filtered.cpu().numpy(), want, "footprint between two runs")
    assert_same(out2.cpu().numpy(), upscale_ref.upscale(s["rgb_lo"], g, s["g_hi"], f, flags=upscale_ref.ALBEDO)[0], "run after")
    # rayz_hip_upscaler_timing after run + footprint still reports the run
    out3 = up.run(x, tl, th, var_rgb=v, flags=capi.DENOISE_ALBEDO)
    torch.cuda.synchronize()
    before = up.timing()
    up.footprint_albedo(tl, th)
    torch.cuda.synchronize()
    assert up.timing() == before and 0 < before[0] < 1000 and 0 < before[1] < 1000
    assert 0 < up.footprint_timing() < 1000
    del out3
    # refused behind the handle: an output overlapping an input, or the other output, without starting where it starts
    need = ("index", "albedo")
    ol, oh = render._gbuffer_pointers(tl, need), render._gbuffer_pointers(th, need)
    out = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    cnt = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def rc(out_ptr, cnt_ptr=None):
        return lib.rayz_hip_upscaler_footprint_albedo(up._h, C.byref(ol), C.byref(oh), C.c_void_p(out_ptr), C.c_void_p(cnt_ptr), None)

    assert rc(th.albedo.data_ptr() + 12) == capi.ERR_BAD_ARG and b"aliases" in lib.rayz_hip_last_error()
    assert rc(tl.albedo.data_ptr() + 4) == capi.ERR_BAD_ARG and b"aliases" in lib.rayz_hip_last_error()
    assert rc(out.data_ptr(), th.index.data_ptr() + 1) == capi.ERR_BAD_ARG and b"aliases" in lib.rayz_hip_last_error()
    assert rc(out.data_ptr(), out.data_ptr() + 5) == capi.ERR_BAD_ARG and b"aliases" in lib.rayz_hip_last_error()
    assert rc(out.data_ptr(), cnt.data_ptr()) == capi.OK  # through the C ABI
    torch.cuda.synchronize()
    assert_same(out.cpu().numpy(), want, "through the C ABI")
    assert np.array_equal(cnt.cpu().numpy(), want_count)
    with pytest.raises(ValueError, match="must be"):
        up.footprint_albedo(tl, th, out=torch.empty((h, w + 1, 3), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="must be"):
        up.footprint_albedo(tl, th, count=torch.empty((h, w), dtype=torch.int32, device="cuda"))
    up.close()


def test_defaults_and_python_errors(gpu):
    """run(footprint=False) is what it was, bit for bit, and the default; footprint=True with phase= or without DENOISE_ALBEDO
    raises ValueError before anything is launched."""
    w, h, f = 17, 9, 2
    s = footprint_scenes.pair(w, h, f, 1)
    up = render.Upscaler(f * w, f * h, f)
    x, v = torch.from_numpy(s["rgb_lo"].copy()).cuda(), torch.from_numpy(s["var_lo"].copy()).cuda()
    tl, th = to_gbuffer(s["g_lo"]), to_gbuffer(s["g_hi"])
    for prm in (dict(), dict(flags=capi.DENOISE_ALBEDO)):
        flags = prm.get("flags", capi.UPSCALE_DEFAULTS["flags"])
        want = upscale_ref.upscale(s["rgb_lo"], s["g_lo"], s["g_hi"], f, var_rgb=s["var_lo"], flags=flags)
        for kw in (dict(), dict(footprint=False)):
            out, var, stage = up.run(x, tl, th, var_rgb=v, stage=True, **prm, **kw)
            torch.cuda.synchronize()
            assert_same(out.cpu().numpy(), want[0], f"{prm} {kw} colour")
            assert_same(var.cpu().numpy(), want[1], f"{prm} {kw} variance")
            assert np.array_equal(stage.cpu().numpy(), want[2])
    assert capi.UPSCALE_DEFAULTS["flags"] == 0
    with pytest.raises(ValueError, match="phase"):
        up.run(x, tl, th, footprint=True, phase=(0, 0), flags=capi.DENOISE_ALBEDO)
    with pytest.raises(ValueError, match="DENOISE_ALBEDO"):
        up.run(x, tl, th, footprint=True)
    with pytest.raises(ValueError, match="DENOISE_ALBEDO"):
        up.run(x, tl, th, footprint=True, flags=0)
    with pytest.raises(capi.RayzHipError):  # nothing was launched by the refused calls
        up.footprint_timing()
    up.close()


def test_a_rendered_pair(gpu):
    """The three-spheres scene under the library's own G-buffers at 48x27 and 96x54 (f = 2): the device equals the mirror, the
    checkered ground's albedo moves, and the composed run equals the upscale mirror on the filtered albedo."""
    t = tracer.threeSpheres(96, seed=3)
    t.samples_per_px, t.max_bounces = 4, 8
    t.set_gpu(render_seed=17, chunk_spp=4)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    p.traversal, p.tmin = capi.TRAVERSAL_BVH, 1e-3
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
    host = lambda g: upscale_ref.Guides(*(getattr(g, k).cpu().numpy() for k in ("index", "normal", "point", "albedo")))  # noqa: E731
    h_lo, h_hi = host(g_lo), host(g_hi)
    want, want_count = footprint_ref.footprint_guides(h_lo, h_hi, f)
    up = render.Upscaler(96, 54, f)
    got, n = up.footprint_albedo(g_lo, g_hi, count=True)
    torch.cuda.synchronize()
    assert_same(got.cpu().numpy(), want, "rendered pair albedo")
    assert np.array_equal(n.cpu().numpy(), want_count)
    assert (want_count < 4).any() and (want_count == 4).any()  # silhouettes: blocks that match partly
    out = up.run(frame, g_lo, g_hi, footprint=True, flags=capi.DENOISE_ALBEDO)
    torch.cuda.synchronize()
    g = upscale_ref.Guides(h_lo.index, h_lo.normal, h_lo.point, want)
    assert_same(out.cpu().numpy(), upscale_ref.upscale(frame.cpu().numpy(), g, h_hi, f, flags=upscale_ref.ALBEDO)[0], "rendered pair composed run")
    up.close()
    ds.close()
