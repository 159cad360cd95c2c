"""Temporal accumulation's moments mode on the GPU (rayz_hip_temporal_track_moments / _step_moments, `render.Temporal(moments=True)`;
DESIGN.md §4.16): every colour, variance, history length and W2 of every step equals the CPU restatement
(tests/temporal_moments_mirror.cpp) bit for bit — sequences that start, stay static, move by a fraction of a pixel and move again,
through an exact camera and a general one, at sizes of one pixel, smaller than the halo, no tile multiple and several tiles in both
directions, at the defaults and with w2_max and min_taps at their ends, with and without the optional outputs; the hand-derived
exact answers of tests/temporal_moments_cases.py; a plain and a moments handle interleaved on one stream; the rules of changing a
handle's kind; a handle destroyed after its stream; and end to end on one-chunk frames under a panning camera."""
import ctypes as C

import numpy as np
import pytest
import torch

import temporal_cases
import temporal_moments_cases as cases
import temporal_moments_ref as ref
import temporal_ref
from rayz_amd import capi, render, tracer

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 3), (33, 9), (45, 23), (97, 41)]  # (width, height)
ORIGINS = [(0, 0), (0, 0), (0.25, -0.625), (1.25, 0.375)]  # first, static, a fractional move, a move by (1, 1) from there
PARAMS = [{}, dict(w2_max=0.0), dict(w2_max=1.0), dict(min_taps=2.0), dict(min_taps=49.0)]
NAMES = ("colour", "variance", "length", "W2")


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ; first at {bad[:5].tolist()}: " \
                          f"{[(got[tuple(b)], want[tuple(b)]) for b in bad[:3]]}"


def camera_desc(cam):
    return capi.CameraDesc(**{k: tuple(float(x) for x in cam[k]) for k in ("look_from", "px_du", "px_dv", "px_origin")})


def to_gbuffer(index, normal, point):
    g = render.QueryResult()
    g.index, g.normal, g.point = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (index, normal, point))
    return g


def gpu_step(tm, rgb, index, normal, point, camera, spp, optional=True, **prm):
    """One moments step from numpy arrays; returns (rgb, var, length, w2) as numpy, or (rgb, var) without the optional outputs.
    Checks that the colour input and the guides are left as they were."""
    x = torch.from_numpy(rgb).cuda()
    g = to_gbuffer(index, normal, point)
    res = tm.step_moments(x, g, camera_desc(camera), spp, length=optional, w2=optional, **prm)
    torch.cuda.synchronize()
    assert len(res) == (4 if optional else 2)
    assert np.array_equal(x.cpu().numpy().view(np.uint32), rgb.view(np.uint32)), "the step changed its colour input"
    for got, was in ((g.index, index), (g.normal, normal), (g.point, point)):
        assert np.array_equal(got.cpu().numpy(), was), "the step changed its G-buffer"
    return tuple(r.cpu().numpy() for r in res)


def frame_args(f):
    return f["rgb"], f["index"], f["normal"], f["point"], f["camera"]


def run_sequence(frames, w, h, what, **prm):
    """The frames through the mirror and through two device handles — with the optional outputs and without them."""
    mirror = ref.TemporalMoments(w, h)
    a, b = render.Temporal(w, h, moments=True), render.Temporal(w, h, moments=True)
    for k, f in enumerate(frames):
        want = mirror.step(*frame_args(f), 8, **prm)
        got = gpu_step(a, *frame_args(f), 8, **prm)
        for name, x, y in zip(NAMES, got, want):
            same_bits(x, y, f"{what} step {k} {name}")
        got = gpu_step(b, *frame_args(f), 8, optional=False, **prm)
        same_bits(got[0], want[0], f"{what} step {k} colour, no optional outputs")
        same_bits(got[1], want[1], f"{what} step {k} variance, no optional outputs")
        assert all(np.isfinite(x).all() for x in want) and (want[3] > 0).all() and (want[3] <= 1).all()
    assert a.timing() > 0
    a.close(), b.close()
    return mirror


@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_the_mirror(gpu, w, h):
    """First, static, a fractional move and a further move, on one synthetic world through the exact camera: each step's outputs, and
    through the following step the history it left; at the defaults, with w2_max 0 (the spatial estimate always) and 1 (never), and
    with min_taps 2 and 49."""
    frames = temporal_cases.plane_sequence(w, h, 100 * w + h, ORIGINS)
    for prm in PARAMS:
        m = run_sequence(frames, w, h, f"{w}x{h} {prm}", **prm)
        assert not m.last_static


@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_the_mirror_through_a_general_camera(gpu, w, h):
    """A camera whose matrix, projection and bilinear weights all round: still bit for bit, with alpha_min and n_max binding too."""
    frames = temporal_cases.general_sequence(w, h, 5 * w + h)
    for prm in PARAMS + [dict(alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)]:
        m = run_sequence(frames, w, h, f"{w}x{h} general {prm}", **prm)
    if w * h > 100:
        hit = frames[-1]["index"] >= 0
        assert not m.last_static and (m.state()[4][..., 3][hit] < 1).mean() > 0.5  # blended values, not the input passed through


def test_device_gives_the_hand_derived_answers(gpu):
    """Every case of tests/temporal_moments_cases.py against its RATIONAL expectation directly — not through the mirror."""
    def step(tm, s):
        return gpu_step(tm, s.rgb, s.index, s.normal, s.point, s.camera, s.spp, **s.params)

    for c in cases.cases():
        h, w = c.steps[0].index.shape
        tm = render.Temporal(w, h, moments=True)
        out = c.run(tm, step)
        c.check(*out, "device")
        assert all(np.isfinite(a).all() for a in out)
        tm.close()


def test_a_plain_and_a_moments_handle_interleaved_on_one_stream(gpu):
    """Steps of a plain handle and of a moments handle alternating on one stream give what each gives alone (its mirror)."""
    w, h = 97, 41
    frames = temporal_cases.plane_sequence(w, h, 4197, ORIGINS)
    plain, mom = render.Temporal(w, h), render.Temporal(w, h, moments=True)
    want_p, want_m = temporal_ref.Temporal(w, h), ref.TemporalMoments(w, h)
    inputs = [(torch.from_numpy(f["rgb"]).cuda(), torch.from_numpy(f["var"]).cuda(), to_gbuffer(f["index"], f["normal"], f["point"]),
               camera_desc(f["camera"])) for f in frames]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    keep = [(plain.step(x, v, g, cam, 8, length=True, stream=s.cuda_stream),
             mom.step_moments(x, g, cam, 8, length=True, w2=True, stream=s.cuda_stream)) for x, v, g, cam in inputs]
    s.synchronize()
    for k, (f, (rp, rm)) in enumerate(zip(frames, keep)):
        for name, x, y in zip(NAMES, rp, want_p.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], 8)):
            same_bits(x.cpu().numpy(), y, f"plain step {k} {name}")
        for name, x, y in zip(NAMES, rm, want_m.step(*frame_args(f), 8)):
            same_bits(x.cpu().numpy(), y, f"moments step {k} {name}")
    plain.close(), mom.close()


def test_a_handle_changes_kind_only_without_history(gpu):
    w, h = 33, 9
    frames = temporal_cases.plane_sequence(w, h, 12, ORIGINS[:2])
    f = frames[0]
    x, v, g = torch.from_numpy(f["rgb"]).cuda(), torch.from_numpy(f["var"]).cuda(), to_gbuffer(f["index"], f["normal"], f["point"])
    cam = camera_desc(f["camera"])
    tm = render.Temporal(w, h)
    with pytest.raises(capi.RayzHipError, match="plain temporal handle"):
        tm.step_moments(x, g, cam, 8)
    tm.step(x, v, g, cam, 8)
    with pytest.raises(capi.RayzHipError, match="has history"):
        tm.track_moments()
    tm.step(x, v, g, cam, 8)  # still a plain handle
    tm.reset()
    tm.track_moments()
    tm.track_moments()  # a second call does nothing
    with pytest.raises(capi.RayzHipError, match="moments mode"):
        tm.step(x, v, g, cam, 8)
    with pytest.raises(ValueError, match="out must not be rgb"):
        tm.step_moments(x, g, cam, 8, out=x)
    with pytest.raises(ValueError, match="unknown temporal parameter"):
        tm.step_moments(x, g, cam, 8, w2max=0.5)
    with pytest.raises(ValueError, match="w2 must be"):
        tm.step_moments(x, g, cam, 8, w2=torch.zeros((h, w, 3), device="cuda"))
    with pytest.raises(capi.RayzHipError, match="min_taps"):
        tm.step_moments(x, g, cam, 8, min_taps=1.0)
    want = ref.TemporalMoments(w, h)
    for fr in frames:  # the handle that changed kind after a reset steps like a fresh one
        got = gpu_step(tm, *frame_args(fr), 8)
        for name, a, b in zip(NAMES, got, want.step(*frame_args(fr), 8)):
            same_bits(a, b, f"after track_moments: {name}")
    tm.reset()  # .. and stays a moments handle across a reset
    got = gpu_step(tm, *frame_args(frames[0]), 8)
    for name, a, b in zip(NAMES, got, ref.TemporalMoments(w, h).step(*frame_args(frames[0]), 8)):
        same_bits(a, b, f"after reset: {name}")
    tm.close()


def test_destroy_after_the_stream_is_gone(gpu):
    """A step on a stream the caller then destroys: the next step and close() wait on the handle's own event, not on that stream."""
    w, h = 97, 41
    frames = temporal_cases.plane_sequence(w, h, 77, ORIGINS[:3])
    want = ref.TemporalMoments(w, h)
    tm = render.Temporal(w, h, moments=True)
    tensors = [(torch.from_numpy(np.ascontiguousarray(f["rgb"])).cuda(), to_gbuffer(f["index"], f["normal"], f["point"])) for f in frames]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    tm.step_moments(tensors[0][0], tensors[0][1], camera_desc(frames[0]["camera"]), 8, stream=s.cuda_stream)
    tm.step_moments(tensors[1][0], tensors[1][1], camera_desc(frames[1]["camera"]), 8, stream=s.cuda_stream)
    del s
    out = tm.step_moments(tensors[2][0], tensors[2][1], camera_desc(frames[2]["camera"]), 8, length=True, w2=True)
    torch.cuda.synchronize()
    for f in frames:
        r = want.step(*frame_args(f), 8)
    for name, x, y in zip(NAMES, out, r):
        same_bits(x.cpu().numpy(), y, f"a step after steps on a released stream: {name}")
    s = torch.cuda.Stream()
    tm.step_moments(tensors[0][0], tensors[0][1], camera_desc(frames[0]["camera"]), 8, stream=s.cuda_stream)
    del s
    tm.close()  # (waits for that step through the handle's event)
    torch.cuda.synchronize()


def panned(cam, pixels):
    """`cam` with px_origin moved by `pixels` pixel steps along px_du: the view pans."""
    c = capi.CameraDesc.from_buffer_copy(cam)
    for j in range(3):
        c.px_origin[j] = cam.px_origin[j] + pixels * cam.px_du[j]
    return c


def test_end_to_end_on_one_chunk_frames_under_a_panning_camera(gpu):
    """threeSpheres at 64x36, six frames of 4 spp in ONE chunk (no tracked handle, no variance input), a seed per frame: static for
    three frames, then a pan of 1.5 pixels per frame.  Camera G-buffer, `Temporal.step_moments` at its defaults, then
    `Denoiser.run_guided` on the step's outputs.  Everything is finite; under the pan more than half of the hit pixels have W2 < 1;
    and on every frame after the first the result is nearer the 512-spp frame of the same camera than the raw frame is — the sign is
    asserted, the ratios are printed."""
    t = tracer.threeSpheres(64, seed=3)
    t.samples_per_px, t.max_bounces = 4, 8
    t.set_gpu(render_seed=17, chunk_spp=0, traversal=capi.TRAVERSAL_BVH, tmin=1e-3)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    w, h = p.width, p.height
    sched = (C.c_uint32 * 8)()
    assert capi.load().rayz_hip_chunk_schedule(C.byref(p), sched, 8) == 1  # one chunk: K = 1
    ds = render.DeviceScene(sd)
    tm, dn = render.Temporal(w, h, moments=True), render.Denoiser(w, h)
    refs = {}
    for k in range(6):
        pan = 1.5 * max(0, k - 2)
        c = panned(cam, pan)
        if pan not in refs:
            q = capi.RenderParams.from_buffer_copy(p)
            q.samples_per_px, q.chunk_spp, q.seed = 512, 0, 999
            big = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ds.render_into(c, q, big.data_ptr())
            ds.sync()
            refs[pan] = big.cpu().numpy().astype(np.float64)
        q = capi.RenderParams.from_buffer_copy(p)
        q.seed = 100 + k
        frame = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ds.render_into(c, q, frame.data_ptr())
        ds.sync()
        g = ds.gbuffer(c, p)
        ds.query_sync()
        out, vout, length, w2 = tm.step_moments(frame, g, c, 4, length=True, w2=True)
        den, dvar = dn.run_guided(out, vout, g, var_out=True)
        torch.cuda.synchronize()
        raw, out_h, vout_h, len_h, w2_h, den_h, dvar_h, idx = (a.cpu().numpy() for a in (frame, out, vout, length, w2, den, dvar, g.index))
        for name, a in (("frame", raw), ("step colour", out_h), ("step variance", vout_h), ("length", len_h), ("W2", w2_h),
                        ("filtered", den_h), ("filtered variance", dvar_h)):
            assert np.isfinite(a).all(), (k, name)
        hit = idx >= 0
        assert hit.any() and (vout_h >= 0).all() and (vout_h <= 2.0 ** 32).all() and (w2_h > 0).all() and (w2_h <= 1).all()
        assert (w2_h[~hit] == 1).all() and (vout_h[~hit] == 0).all() and (len_h[~hit] == 4).all()
        if k == 0:
            assert (w2_h == 1).all()
        elif k < 3:
            assert (len_h[hit] == 4 * (k + 1)).all() and (w2_h[hit] < 1).all(), (k, np.unique(len_h[hit]))
        else:
            share = (w2_h[hit] < 1).mean()
            print(f"frame {k}: {share:.4f} of the hit pixels have W2 < 1")
            assert share > 0.5, (k, share)
        mse = [((a - refs[pan]) ** 2).mean() for a in (raw, out_h, den_h)]
        print(f"frame {k}: MSE against 512 spp raw {mse[0]:.4e}, moments step {mse[1]:.4e} (x{mse[1] / mse[0]:.3f}), "
              f"moments step + guided {mse[2]:.4e} (x{mse[2] / mse[0]:.3f})")
        if k:
            assert mse[2] < mse[0], (k, mse)
    tm.close(), dn.close(), ds.close()
