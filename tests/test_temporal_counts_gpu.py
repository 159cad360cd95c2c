"""Temporal accumulation's counts step on the GPU (rayz_hip_temporal_step_counts / _step_moments_counts, `render.Temporal.step` /
`step_moments` with a tensor for spp): every output of every step equals the CPU restatement
(tests/temporal_counts_mirror.cpp) bit for bit under random per-pixel counts with NaN inputs wherever the count is 0; the
hand-derived answers of tests/temporal_counts_cases.py; uniform counts equal the scalar step; cycling a lattice's phases under a
still camera ends in the whole frame's own step; and what the step refuses."""
import ctypes as C

import numpy as np
import pytest
import torch

import temporal_cases
import temporal_counts_cases as cases
import temporal_counts_ref as ref
from rayz_amd import capi, render
from test_temporal_gpu import SIZES, camera_desc, same_bits, three_spheres, to_gbuffer, tracked_frame
from test_temporal_moments_gpu import PARAMS

pytestmark = pytest.mark.gpu

ORIGINS = [(0, 0), (0, 0), (0.25, -0.625), (1.25, 0.375)]  # first, static, a fractional move, a move by (1, 1) from there
BINDING = dict(alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)
DRAW = np.array([0, 0, 1, 4, 8])
NAN = np.float32(np.nan)


def sparse(frames, seed):
    """The frames with per-pixel counts drawn from {0, 0, 1, 4, 8} and NaN colour and variance wherever the count is 0."""
    rng = np.random.default_rng(seed)
    out = []
    for f in frames:
        counts = rng.choice(DRAW, size=f["index"].shape).astype(np.int32)
        rgb, var = f["rgb"].copy(), f["var"].copy()
        rgb[counts == 0] = NAN
        var[counts == 0] = NAN
        out.append(dict(f, rgb=rgb, var=var, counts=counts))
    return out


def zero_share(frames):
    return float(np.mean([(f["counts"] == 0).mean() for f in frames]))


def tensors(f, moments):
    return ([torch.from_numpy(f["rgb"]).cuda()] + ([] if moments else [torch.from_numpy(f["var"]).cuda()]),
            to_gbuffer(f["index"], f["normal"], f["point"]), torch.from_numpy(np.ascontiguousarray(f["counts"], dtype=np.int32)).cuda())


def plain_step(tm, f, in_place=False, length=True, **prm):
    (x, v), g, c = tensors(f, False)
    res = tm.step(x, v, g, camera_desc(f["camera"]), c, out=x if in_place else None, var_out=v if in_place else None, length=length, **prm)
    torch.cuda.synchronize()
    assert np.array_equal(c.cpu().numpy(), f["counts"]), "the step changed its counts"
    if not in_place:
        assert np.array_equal(x.cpu().numpy().view(np.uint32), f["rgb"].view(np.uint32)), "an out-of-place step changed its colour input"
    return tuple(r.cpu().numpy() for r in res)


def moments_step(tm, f, optional=True, **prm):
    (x,), g, c = tensors(f, True)
    res = tm.step_moments(x, g, camera_desc(f["camera"]), c, length=optional, w2=optional, **prm)
    torch.cuda.synchronize()
    assert np.array_equal(c.cpu().numpy(), f["counts"]), "the step changed its counts"
    assert np.array_equal(x.cpu().numpy().view(np.uint32), f["rgb"].view(np.uint32)), "the step changed its colour input"
    return tuple(r.cpu().numpy() for r in res)


def run_plain(frames, w, h, what, **prm):
    mirror = ref.TemporalCounts(w, h)
    a, b = render.Temporal(w, h), render.Temporal(w, h)
    for k, f in enumerate(frames):
        want = mirror.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], f["counts"], **prm)
        for name, x, y in zip(("colour", "variance", "length"), plain_step(a, f, **prm), want):
            same_bits(x, y, f"{what} step {k} {name}")
        got = plain_step(b, f, in_place=True, length=False, **prm)
        same_bits(got[0], want[0], f"{what} step {k} colour, in place")
        same_bits(got[1], want[1], f"{what} step {k} variance, in place")
        sampled = (mirror.state()[0][..., 3] > 0) & (f["index"] >= 0)  # a record that holds samples holds no NaN
        assert np.isfinite(want[0][sampled]).all() and np.isfinite(want[1]).all()
    a.close(), b.close()
    return mirror


def run_moments(frames, w, h, what, **prm):
    mirror = ref.TemporalMomentsCounts(w, h)
    a, b = render.Temporal(w, h, moments=True), render.Temporal(w, h, moments=True)
    for k, f in enumerate(frames):
        want = mirror.step(f["rgb"], f["index"], f["normal"], f["point"], f["camera"], f["counts"], **prm)
        for name, x, y in zip(("colour", "variance", "length", "W2"), moments_step(a, f, **prm), want):
            same_bits(x, y, f"{what} step {k} {name}")
        got = moments_step(b, f, optional=False, **prm)
        same_bits(got[0], want[0], f"{what} step {k} colour, no optional outputs")
        same_bits(got[1], want[1], f"{what} step {k} variance, no optional outputs")
        sampled = (mirror.state()[0][..., 3] > 0) & (f["index"] >= 0)
        assert np.isfinite(want[0][sampled]).all() and (want[1] >= 0).all() and (want[1] <= 2.0 ** 32).all()
    a.close(), b.close()
    return mirror


@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_the_mirror(gpu, w, h):
    """First, static, a fractional move and a further move through the exact camera, at the defaults and with alpha_min, n_max and
    the surface tests binding: out of place with the length, in place without it."""
    frames = sparse(temporal_cases.plane_sequence(w, h, 100 * w + h, ORIGINS), 7 * w + h)
    if w * h > 100:
        assert 0.2 < zero_share(frames) < 0.6, zero_share(frames)
    m = run_plain(frames, w, h, f"{w}x{h} defaults")
    run_plain(frames, w, h, f"{w}x{h} binding", **BINDING)
    if w * h > 100:
        hit = frames[-1]["index"] >= 0
        n = m.state()[0][..., 3]
        assert ((n > 8) & hit).any() and ((frames[-1]["counts"] == 0) & (n > 0) & hit).any()  # blended, and kept without a sample


@pytest.mark.parametrize("w,h", [(45, 23), (97, 41)])
def test_device_equals_the_mirror_through_a_general_camera(gpu, w, h):
    frames = sparse(temporal_cases.general_sequence(w, h, 5 * w + h), 3 * w + h)
    assert 0.2 < zero_share(frames) < 0.6, zero_share(frames)
    run_plain(frames, w, h, f"{w}x{h} general")
    run_plain(frames, w, h, f"{w}x{h} general binding", **BINDING)


@pytest.mark.parametrize("w,h", SIZES)
def test_moments_device_equals_the_mirror(gpu, w, h):
    """.. the moments handle, with length and W2 and without: at the defaults, with w2_max 0 (the neighbourhood of sampled positions
    always) and 1 (never), and with min_taps 2 and 49."""
    frames = sparse(temporal_cases.plane_sequence(w, h, 100 * w + h, ORIGINS), 11 * w + h)
    if w * h > 100:
        assert 0.2 < zero_share(frames) < 0.6, zero_share(frames)
    for prm in PARAMS:
        run_moments(frames, w, h, f"{w}x{h} {prm}", **prm)


@pytest.mark.parametrize("w,h", [(45, 23), (97, 41)])
def test_moments_device_equals_the_mirror_through_a_general_camera(gpu, w, h):
    frames = sparse(temporal_cases.general_sequence(w, h, 5 * w + h), 13 * w + h)
    assert 0.2 < zero_share(frames) < 0.6, zero_share(frames)
    for prm in PARAMS + [BINDING]:
        run_moments(frames, w, h, f"{w}x{h} general {prm}", **prm)


def test_device_gives_the_hand_derived_answers(gpu):
    """Every case of tests/temporal_counts_cases.py against its RATIONAL expectation directly — not through the mirror."""
    for c in cases.cases():
        h, w = c.steps[0].index.shape
        tm = render.Temporal(w, h)
        out = c.run(tm, lambda t, s: plain_step(t, dict(rgb=s.rgb, var=s.var, index=s.index, normal=s.normal, point=s.point,
                                                        camera=s.camera, counts=s.counts), **s.params))
        c.check(*out, "device")
        tm.close()
    for c in cases.moments_cases():
        h, w = c.steps[0].index.shape
        tm = render.Temporal(w, h, moments=True)
        out = c.run(tm, lambda t, s: moments_step(t, dict(rgb=s.rgb, index=s.index, normal=s.normal, point=s.point, camera=s.camera,
                                                          counts=s.counts), **s.params))
        c.check(*out, "device")
        tm.close()


def test_uniform_counts_equal_the_scalar_step(gpu):
    """Two handles on one plane sequence, one stepped with spp = 8 and one with a tensor of 8s: bit for bit, plain and moments."""
    w, h = 97, 41
    frames = temporal_cases.plane_sequence(w, h, 4197, ORIGINS)
    eight = torch.full((h, w), 8, dtype=torch.int32, device="cuda")
    for moments in (False, True):
        a, b = render.Temporal(w, h, moments=moments), render.Temporal(w, h, moments=moments)
        for k, f in enumerate(frames):
            ins, g, _ = tensors(dict(f, counts=np.zeros((h, w), np.int32)), moments)
            cam = camera_desc(f["camera"])
            extra = dict(length=True, w2=True) if moments else dict(length=True)
            step = (lambda t, spp: t.step_moments(*ins, g, cam, spp, **extra)) if moments else (lambda t, spp: t.step(*ins, g, cam, spp, **extra))
            ra, rb = step(a, 8), step(b, eight)
            torch.cuda.synchronize()
            for x, y in zip(ra, rb):
                same_bits(x.cpu().numpy(), y.cpu().numpy(), f"moments={moments} step {k}")
        a.close(), b.close()


def whole_frame(ds, cam, p, seed):
    """One whole frame of p's samples in one piece, as a one-chunk or one-shot caller has it."""
    q = capi.RenderParams.from_buffer_copy(p)
    q.seed = seed
    frame = torch.empty((p.height, p.width, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ds.render_into(cam, q, frame.data_ptr())
    ds.sync()
    return frame


def lattice_phase(ds, cam, p, seed, f, phase, var):
    """The phase's lattice pixels of that frame, traced sparsely into NaN-filled full frames: (frame, variance or None, counts)."""
    q = capi.RenderParams.from_buffer_copy(p)
    q.seed = seed
    pixels, _ = render.lattice_pixels(p.width, p.height, f, phase, device="cuda")
    frame = torch.full((p.height, p.width, 3), float("nan"), dtype=torch.float32, device="cuda")
    res = ds.render_pixels(cam, q, pixels, dest=pixels, out=frame, var=var)
    ds.sync()
    return frame, (res[1] if var else None), render.lattice_counts(p.width, p.height, f, phase, p.samples_per_px, device="cuda")


@pytest.mark.parametrize("f", [2, 4])
def test_a_phase_cycle_ends_in_the_whole_frames_step(gpu, f):
    """threeSpheres at 64x36, 8 spp in two chunks, still camera.  Every phase of an every-f-th-pixel lattice is traced sparsely into
    NaN-filled frames and stepped with its counts; after the f² steps of a cycle the output, the variance and the length equal, on
    hit pixels and bit for bit, ONE scalar step of the whole tracked frame — and after a second cycle from another seed the second
    whole-frame step."""
    t, sd, cam, p = three_spheres(8, 4)
    w, h = p.width, p.height
    ds = render.DeviceScene(sd)
    g = ds.gbuffer(cam, p)
    ds.query_sync()
    hit = (g.index >= 0).cpu().numpy()
    assert 0.2 < hit.mean() <= 1.0
    whole, cycled = render.Temporal(w, h), render.Temporal(w, h)
    for cycle, seed in enumerate((41, 97)):
        frame, var = tracked_frame(ds, cam, p, seed)
        want = whole.step(frame, var, g, cam, 8, length=True)
        for phase in render.phase_sequence(f):
            x, v, counts = lattice_phase(ds, cam, p, seed, f, phase, True)
            got = cycled.step(x, v, g, cam, counts, length=True)
        torch.cuda.synchronize()
        for name, a, b in zip(("colour", "variance", "length"), got, want):
            same_bits(a.cpu().numpy()[hit], b.cpu().numpy()[hit], f"f={f} cycle {cycle} {name}")
        assert (want[2].cpu().numpy()[hit] == 8 * (cycle + 1)).all()
    whole.close(), cycled.close(), ds.close()


@pytest.mark.parametrize("f", [2, 4])
def test_a_phase_cycle_of_a_moments_handle(gpu, f):
    """The same on one-chunk frames through a moments handle: colour, length and W2 are held bit for bit; the variance differs by
    construction (a lattice step's neighbourhood holds the phase's pixels only) and is finite and in [0, 2^32]."""
    t, sd, cam, p = three_spheres(8, 8)
    w, h = p.width, p.height
    ds = render.DeviceScene(sd)
    g = ds.gbuffer(cam, p)
    ds.query_sync()
    hit = (g.index >= 0).cpu().numpy()
    whole, cycled = render.Temporal(w, h, moments=True), render.Temporal(w, h, moments=True)
    for cycle, seed in enumerate((41, 97)):
        want = whole.step_moments(whole_frame(ds, cam, p, seed), g, cam, 8, length=True, w2=True)
        for phase in render.phase_sequence(f):
            x, _, counts = lattice_phase(ds, cam, p, seed, f, phase, False)
            got = cycled.step_moments(x, g, cam, counts, length=True, w2=True)
        torch.cuda.synchronize()
        for k, name in ((0, "colour"), (2, "length"), (3, "W2")):
            same_bits(got[k].cpu().numpy()[hit], want[k].cpu().numpy()[hit], f"f={f} cycle {cycle} {name}")
        v = got[1].cpu().numpy()[hit]
        assert np.isfinite(v).all() and (v >= 0).all() and (v <= 2.0 ** 32).all()
    whole.close(), cycled.close(), ds.close()


def test_refusals(gpu):
    w, h = 33, 9
    f = sparse(temporal_cases.plane_sequence(w, h, 1, ORIGINS[:1]), 2)[0]
    (x, v), g, counts = tensors(f, False)
    cam = camera_desc(f["camera"])
    fb = render.Temporal(w, h, moments=True, feedback=True)
    with pytest.raises(capi.RayzHipError, match=rf"status {capi.ERR_STATE}\).*feedback"):
        fb.step_moments(x, g, cam, counts)
    fb.step_moments(x.nan_to_num(), g, cam, 8)  # (the handle is as it was: the scalar step still runs)
    fb.close()
    tm = render.Temporal(w, h)
    for bad, what in ((counts.to(torch.int64), "must be torch.int32"), (counts[:, :-1].contiguous(), "must be"), (counts.cpu(), "GPU memory"),
                      (counts.float(), "must be torch.int32"), (-counts - 1, "negative")):
        with pytest.raises(ValueError, match=what):
            tm.step(x, v, g, cam, bad)
    lib = capi.load()
    o = render._gbuffer_pointers(g, ["index", "normal", "point"])
    out, vout, lout = (torch.empty_like(x), torch.empty_like(v), torch.empty((h, w), device="cuda"))
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def plain(c, length=None):
        return lib.rayz_hip_temporal_step_counts(tm._h, None, C.byref(cam), c, p(x), p(v), C.byref(o), p(out), p(vout), length, None)

    assert plain(None) == capi.ERR_BAD_ARG and b"counts" in lib.rayz_hip_last_error()
    assert plain(p(out)) == capi.ERR_BAD_ARG and plain(p(vout)) == capi.ERR_BAD_ARG and plain(p(lout), p(lout)) == capi.ERR_BAD_ARG
    assert b"output" in lib.rayz_hip_last_error()
    mm = render.Temporal(w, h, moments=True)

    def moments(handle, c, length=None, w2=None):
        return lib.rayz_hip_temporal_step_moments_counts(handle, None, None, C.byref(cam), c, p(x), C.byref(o), p(out), p(vout), length, w2, None)

    assert moments(mm._h, None) == capi.ERR_BAD_ARG
    assert moments(mm._h, p(out)) == capi.ERR_BAD_ARG and moments(mm._h, p(lout), None, p(lout)) == capi.ERR_BAD_ARG
    assert moments(tm._h, p(counts)) == capi.ERR_STATE and plain(p(counts)) == capi.OK  # a plain handle takes the plain counts step only
    assert lib.rayz_hip_temporal_step_counts(mm._h, None, C.byref(cam), p(counts), p(x), p(v), C.byref(o), p(out), p(vout), None, None) == capi.ERR_STATE
    torch.cuda.synchronize()
    tm.close(), mm.close()
