"""Temporal accumulation on the GPU (rayz_hip_temporal_*, `render.Temporal`): every colour, variance and history
length of every step equals the CPU restatement (tests/temporal_mirror.cpp) bit for bit — sequences that start, stay static, move by
a fraction of a pixel and move again (so the state a step leaves is read back), on synthetic guides seen through an exact camera and
through a general one, variances spanning 0, tiny, large, +inf and NaN, at sizes of one pixel, less than a tile, no tile multiple and
several tiles, with and without the length output, in place and out of place; the hand-derived exact answers of
tests/temporal_cases.py; two handles, reset and replay, a denoiser and a progressive handle undisturbed between steps, a handle
destroyed after its stream; and end to end from tracked progressive handles under a panning camera."""
import numpy as np
import pytest
import torch

import temporal_cases
import temporal_ref
from rayz_amd import capi, render, tracer

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 3), (33, 9), (45, 23), (97, 41)]  # (width, height)
ORIGINS = [(0, 0), (0, 0), (0.25, -0.625), (1.25, 0.375)]  # first, static, a fractional move, a move by (1, 1) from there


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


def gpu_step(tm, rgb, var, index, normal, point, camera, spp, in_place=False, length=True, **prm):
    """One step from numpy arrays; returns (rgb, var, length or None) as numpy.  Checks that the guides, and out of place the
    colour and the variance, are left as they were."""
    x, v = torch.from_numpy(rgb).cuda(), torch.from_numpy(var).cuda()
    g = to_gbuffer(index, normal, point)
    res = tm.step(x, v, g, camera_desc(camera), spp, out=x if in_place else None, var_out=v if in_place else None, length=length, **prm)
    torch.cuda.synchronize()
    if not in_place:
        assert np.array_equal(x.cpu().numpy().view(np.uint32), rgb.view(np.uint32)), "an out-of-place step changed its colour input"
        assert np.array_equal(v.cpu().numpy().view(np.uint32), var.view(np.uint32)), "an out-of-place step changed its variance input"
    for got, was in ((g.index, index), (g.normal, normal), (g.point, point)):
        assert np.array_equal(got.cpu().numpy(), was), "the step changed its G-buffer"
    return res[0].cpu().numpy(), res[1].cpu().numpy(), res[2].cpu().numpy() if length else None


def frame_args(f):
    return f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"]


def run_sequence(frames, w, h, what, **prm):
    """The frames through the mirror and through two device handles — out of place with the length, in place without it."""
    mirror = temporal_ref.Temporal(w, h)
    a, b = render.Temporal(w, h), render.Temporal(w, h)
    for k, f in enumerate(frames):
        want = mirror.step(*frame_args(f), 8, **prm)
        got = gpu_step(a, *frame_args(f), 8, **prm)
        for name, x, y in zip(("colour", "variance", "length"), got, want):
            same_bits(x, y, f"{what} step {k} {name}")
        got = gpu_step(b, *frame_args(f), 8, in_place=True, length=False, **prm)
        assert got[2] is None
        same_bits(got[0], want[0], f"{what} step {k} colour, in place")
        same_bits(got[1], want[1], f"{what} step {k} variance, in place")
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
    assert a.timing() > 0
    a.close(), b.close()
    return mirror


@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_the_mirror(gpu, w, h):
    """First, static, a fractional move and a further move, on one synthetic world through the exact camera: each step's outputs, and
    through the following step the history it left, at the defaults and with alpha_min and n_max binding."""
    frames = temporal_cases.plane_sequence(w, h, 100 * w + h, ORIGINS)
    m = run_sequence(frames, w, h, f"{w}x{h} defaults")
    assert not m.last_static
    run_sequence(frames, w, h, f"{w}x{h} binding", alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)


@pytest.mark.parametrize("w,h", [(45, 23), (97, 41)])
def test_device_equals_the_mirror_through_a_general_camera(gpu, w, h):
    """A camera whose matrix, projection and bilinear weights all round: the device still equals the mirror bit for bit, and the moved
    step finds history for most hit pixels (so the comparison is of blended values, not of the input passed through)."""
    frames = temporal_cases.general_sequence(w, h, 5 * w + h)
    m = run_sequence(frames, w, h, f"{w}x{h} general")
    hit = frames[-1]["index"] >= 0
    assert not m.last_static and (m.state()[0][..., 3][hit] > 8).mean() > 0.5


def test_device_gives_the_hand_derived_answers(gpu):
    """Every case of tests/temporal_cases.py against its RATIONAL expectation directly — not through the mirror."""
    def step(tm, s):
        return gpu_step(tm, s.rgb, s.var, s.index, s.normal, s.point, s.camera, s.spp, **s.params)

    for c in temporal_cases.cases():
        h, w = c.steps[0].index.shape
        tm = render.Temporal(w, h)
        rgb, var, length = c.run(tm, step)
        c.check(rgb, var, length, "device")
        assert np.isfinite(rgb).all() and np.isfinite(var).all() and np.isfinite(length).all()
        tm.close()


def test_two_handles_agree_and_reset_replays(gpu):
    w, h = 97, 41
    frames = temporal_cases.plane_sequence(w, h, 4197, ORIGINS)
    a, b = render.Temporal(w, h), render.Temporal(w, h)
    first = []
    for f in frames:
        ra, rb = gpu_step(a, *frame_args(f), 8), gpu_step(b, *frame_args(f), 8, in_place=True)
        for x, y in zip(ra, rb):
            same_bits(x, y, "two handles")
        first.append(ra)
    assert (first[1][2][frames[1]["index"] >= 0] == 16).all()
    a.reset()
    for f, want in zip(frames, first):
        for x, y in zip(gpu_step(a, *frame_args(f), 8), want):
            same_bits(x, y, "replay after reset")
    with pytest.raises(ValueError, match="var_rgb must be"):
        a.step(torch.zeros((h, w, 3), device="cuda"), torch.zeros((h, w), device="cuda"), to_gbuffer(*frame_args(frames[0])[2:5]),
               camera_desc(frames[0]["camera"]), 8)
    with pytest.raises(ValueError, match="unknown temporal parameter"):
        a.step(torch.zeros((h, w, 3), device="cuda"), torch.zeros((h, w, 3), device="cuda"), to_gbuffer(*frame_args(frames[0])[2:5]),
               camera_desc(frames[0]["camera"]), 8, alpha=0.5)
    with pytest.raises(capi.RayzHipError, match="alpha_min"):
        a.step(torch.zeros((h, w, 3), device="cuda"), torch.zeros((h, w, 3), device="cuda"), to_gbuffer(*frame_args(frames[0])[2:5]),
               camera_desc(frames[0]["camera"]), 8, alpha_min=2.0)
    a.close(), b.close()
    fresh = render.Temporal(4, 4)
    with pytest.raises(capi.RayzHipError, match="no temporal step"):
        fresh.timing()
    fresh.close()


def three_spheres(spp, chunk_spp):
    t = tracer.threeSpheres(64, seed=3)
    t.samples_per_px, t.max_bounces = spp, 8
    t.set_gpu(render_seed=17, chunk_spp=chunk_spp, traversal=capi.TRAVERSAL_BVH, tmin=1e-3)
    return t, t.scene_desc(), t.camera_desc(), t.params()


def panned(cam, pixels):
    """`cam` with px_origin moved by `pixels` pixel steps along px_du: the view pans."""
    c = capi.CameraDesc.from_buffer_copy(cam)
    for j in range(3):
        c.px_origin[j] = cam.px_origin[j] + pixels * cam.px_du[j]
    return c


def tracked_frame(ds, cam, p, seed):
    """One frame of p.samples_per_px samples from a tracked progressive handle with its own seed: (frame, noise_rgb)."""
    q = capi.RenderParams.from_buffer_copy(p)
    q.seed = seed
    pr = ds.progressive(cam, q, track_noise=True)
    frame = torch.full((p.height, p.width, 3), float("nan"), device="cuda")
    torch.cuda.synchronize()
    while not pr.done:
        pr.step(0, frame.data_ptr())
    assert pr.chunks_done >= 2
    var = pr.noise_rgb()
    pr.stats()
    pr.close()
    return frame, var


def test_a_denoiser_and_a_progressive_handle_between_steps_are_undisturbed(gpu):
    """A frame rendered by a tracked handle and filtered by a denoiser BETWEEN the steps of a temporal handle equals, bit for bit, the
    same frame made without any temporal handle; and the temporal handle's outputs equal those of one that ran alone."""
    t, sd, cam, p = three_spheres(8, 4)
    w, h = p.width, p.height
    ds = render.DeviceScene(sd)
    g = ds.gbuffer(cam, p)
    ds.query_sync()
    dn = render.Denoiser(w, h)

    def other_work():
        frame, var = tracked_frame(ds, cam, p, 5)
        out, vout = dn.run_guided(frame, var, g, var_out=True)
        torch.cuda.synchronize()
        return [a.cpu().numpy() for a in (frame, var, out, vout)]

    alone = other_work()
    frames = [tracked_frame(ds, panned(cam, 0.75 * k), p, 30 + k) for k in range(3)]
    gs = []
    for k in range(3):
        gs.append(ds.gbuffer(panned(cam, 0.75 * k), p))
        ds.query_sync()
    a, b = render.Temporal(w, h), render.Temporal(w, h)
    for k in range(3):
        ra = a.step(frames[k][0], frames[k][1], gs[k], panned(cam, 0.75 * k), 8, length=True)
        between = other_work()
        for x, y in zip(between, alone):
            same_bits(x, y, f"other handles after step {k}")
        rb = b.step(frames[k][0], frames[k][1], gs[k], panned(cam, 0.75 * k), 8, length=True)
        torch.cuda.synchronize()
        for x, y in zip(ra, rb):
            same_bits(x.cpu().numpy(), y.cpu().numpy(), f"temporal step {k} with and without other work")
    a.close(), b.close(), dn.close(), ds.close()


def test_destroy_after_the_stream_is_gone(gpu):
    """A step on a stream the caller then destroys: the next step and close() wait on the handle's own event, not on that stream."""
    w, h = 97, 41
    frames = temporal_cases.plane_sequence(w, h, 77, ORIGINS[:3])
    want = temporal_ref.Temporal(w, h)
    tm = render.Temporal(w, h)
    tensors = [[torch.from_numpy(np.ascontiguousarray(f[k])).cuda() for k in ("rgb", "var")] + [to_gbuffer(f["index"], f["normal"], f["point"])]
               for f in frames]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    tm.step(tensors[0][0], tensors[0][1], tensors[0][2], camera_desc(frames[0]["camera"]), 8, stream=s.cuda_stream)
    tm.step(tensors[1][0], tensors[1][1], tensors[1][2], camera_desc(frames[1]["camera"]), 8, stream=s.cuda_stream)
    del s
    out = tm.step(tensors[2][0], tensors[2][1], tensors[2][2], camera_desc(frames[2]["camera"]), 8, length=True)
    torch.cuda.synchronize()
    for f in frames:
        ref = want.step(*frame_args(f), 8)
    for x, y in zip(out, ref):
        same_bits(x.cpu().numpy(), y, "a step after steps on a released stream")
    s = torch.cuda.Stream()
    tm.step(tensors[0][0], tensors[0][1], tensors[0][2], camera_desc(frames[0]["camera"]), 8, stream=s.cuda_stream)
    del s
    tm.close()  # (waits for that step through the handle's event)
    torch.cuda.synchronize()


def test_end_to_end_under_a_panning_camera(gpu):
    """threeSpheres at 64x36, six frames of 8 spp in two chunks, each from a tracked progressive handle with its own seed: static for
    three frames, then a pan of 1.5 pixels per frame.  Camera G-buffer, `noise_rgb()`, `Temporal.step` at its defaults, then
    `Denoiser.run_guided` on the step's outputs.  Everything is finite; while static the length is 8·k on hit pixels; once the pan
    starts more than half of the hit pixels still find history (on the CPU restatement with an oracle G-buffer the share is 0.98:
    tests/test_temporal_cpu.py); and on every frame after the first the step's output is nearer the 512-spp frame of the same camera
    than the raw frame is — only the sign is asserted, the ratios are printed (CPU restatement on oracle frames: 0.52, 0.36, 0.25,
    0.16, 0.17)."""
    t, sd, cam, p = three_spheres(8, 4)
    w, h = p.width, p.height
    ds = render.DeviceScene(sd)
    tm, dn = render.Temporal(w, h), render.Denoiser(w, h)
    refs = {}
    ratios = []
    for k in range(6):
        pan = 1.5 * max(0, k - 2)
        c = panned(cam, pan)
        if pan not in refs:
            q = capi.RenderParams.from_buffer_copy(p)
            q.samples_per_px, q.chunk_spp, q.seed = 512, 0, 999
            ref = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ds.render_into(c, q, ref.data_ptr())
            ds.sync()
            refs[pan] = ref.cpu().numpy().astype(np.float64)
        frame, var = tracked_frame(ds, c, p, 100 + k)
        g = ds.gbuffer(c, p)
        ds.query_sync()
        out, vout, length = tm.step(frame, var, g, c, 8, length=True)
        den, dvar = dn.run_guided(out, vout, g, var_out=True)
        torch.cuda.synchronize()
        raw, out_h, vout_h, len_h, den_h, dvar_h, idx = (a.cpu().numpy() for a in (frame, out, vout, length, den, dvar, g.index))
        for name, a in (("frame", raw), ("step colour", out_h), ("step variance", vout_h), ("length", len_h), ("filtered", den_h),
                        ("filtered variance", dvar_h)):
            assert np.isfinite(a).all(), (k, name)
        hit = idx >= 0
        assert hit.any() and (vout_h >= 0).all() and (len_h[~hit] == 8).all()
        if k < 3:
            assert (len_h[hit] == 8 * (k + 1)).all(), (k, np.unique(len_h[hit]))
        else:
            share = (len_h[hit] > 8).mean()
            print(f"frame {k}: {share:.4f} of the hit pixels found history")
            assert share > 0.5, (k, share)
        mse = [((a - refs[pan]) ** 2).mean() for a in (raw, out_h, den_h)]
        print(f"frame {k}: MSE against 512 spp raw {mse[0]:.4e}, temporal {mse[1]:.4e} (x{mse[1] / mse[0]:.3f}), "
              f"temporal + guided {mse[2]:.4e} (x{mse[2] / mse[0]:.3f})")
        if k:
            assert mse[1] < mse[0], (k, mse)
            ratios.append(mse[1] / mse[0])
    print("temporal / raw MSE per frame 1..5:", " ".join(f"{r:.3f}" for r in ratios))
    tm.close(), dn.close(), ds.close()
