"""Temporal accumulation's feedback mode on the GPU (rayz_hip_temporal_track_feedback / _feedback, `render.Temporal(moments=True,
feedback=True)`) and the guided filter's tap (rayz_hip_denoiser_run_guided_tap): every output of every step equals
the CPU restatement (tests/temporal_feedback_mirror.cpp) bit for bit with a feedback image between every two steps — a random frame,
and the tap of a real guided run — through both cameras, at sizes of one pixel, smaller than the halo, no tile multiple and several
tiles both ways, at the defaults and with w2_max at its ends; a feedback handle that is given none equals a moments handle; the
hand-derived exact answers of tests/temporal_feedback_cases.py; the tap against `run_guided(levels=t)` in every level-kernel form;
the state rules; handles interleaved on one stream and a handle destroyed with a feedback pending."""
import numpy as np
import pytest
import torch

import temporal_cases
import temporal_feedback_cases as cases
import temporal_feedback_ref as ref
import temporal_moments_ref
from rayz_amd import capi, render

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (5, 3), (33, 9), (45, 23), (97, 41)]  # (width, height)
ORIGINS = [(0, 0), (0, 0), (0.25, -0.625), (1.25, 0.375)]  # first, static, a fractional move, a move by (1, 1) from there
PARAMS = [{}, dict(w2_max=0.0), dict(w2_max=1.0)]
NAMES = ("colour", "variance", "length", "W2")


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ; first at {bad[:5].tolist()}: " \
                          f"{[(got[tuple(b)], want[tuple(b)]) for b in bad[:3]]}"


def camera_desc(cam):
    return capi.CameraDesc(**{k: tuple(float(x) for x in cam[k]) for k in ("look_from", "px_du", "px_dv", "px_origin")})


def to_gbuffer(index, normal, point, albedo=None):
    g = render.QueryResult()
    g.index, g.normal, g.point = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (index, normal, point))
    if albedo is not None:
        g.albedo = torch.from_numpy(np.ascontiguousarray(albedo)).cuda()
    return g


def gpu_step(tm, rgb, index, normal, point, camera, spp, **prm):
    res = tm.step_moments(torch.from_numpy(rgb).cuda(), to_gbuffer(index, normal, point), camera_desc(camera), spp, length=True, w2=True, **prm)
    torch.cuda.synchronize()
    return tuple(r.cpu().numpy() for r in res)


def gpu_feedback(tm, image):
    x = torch.from_numpy(np.ascontiguousarray(image)).cuda()
    tm.feedback(x)
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy().view(np.uint32), image.view(np.uint32)), "the feedback changed its input"


def host(*tensors):
    """The tensors on the host, after everything enqueued on the device has finished (the library's stream is not torch's)."""
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in tensors)


def frame_args(f):
    return f["rgb"], f["index"], f["normal"], f["point"], f["camera"]


def random_image(w, h, seed):
    """A frame of the colours' range with a NaN and a +inf pixel where the frame has room for them."""
    rng = np.random.default_rng(seed)
    img = rng.random((h, w, 3), dtype=np.float32) * np.float32(2)
    if w * h > 4:
        img[h // 2, w // 2, 1] = np.nan
        img[0, w - 1, 2] = np.inf
    return img


def run_with_feedback(frames, w, h, what, image_of, **prm):
    """The frames through the mirror and a device handle, image_of(k, device outputs, frame) fed back to both behind every step."""
    mirror, tm = ref.TemporalFeedback(w, h), render.Temporal(w, h, moments=True, feedback=True)
    for k, f in enumerate(frames):
        want = mirror.step(*frame_args(f), 8, **prm)
        got = gpu_step(tm, *frame_args(f), 8, **prm)
        for name, x, y in zip(NAMES, got, want):
            same_bits(x, y, f"{what} step {k} {name}")
        img = image_of(k, got, f)
        mirror.feedback(img)
        gpu_feedback(tm, img)
    assert tm.timing() > 0
    tm.close()


def both_cameras(w, h):
    yield "plane", temporal_cases.plane_sequence(w, h, 100 * w + h, ORIGINS)
    yield "general", temporal_cases.general_sequence(w, h, 5 * w + h) + temporal_cases.general_sequence(w, h, 5 * w + h, shifts=((2.37, 1.61),))


@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_the_mirror_with_a_random_frame_fed_back(gpu, w, h):
    """First, static, a fractional move and a further move; behind every step a random image (with a NaN and a +inf pixel) replaces
    the colour history, so from the second step on colour and m1 differ everywhere, and every later output shows what the write did."""
    for kind, frames in both_cameras(w, h):
        for prm in PARAMS:
            run_with_feedback(frames, w, h, f"{w}x{h} {kind} {prm}", lambda k, got, f: random_image(w, h, 31 * k + w), **prm)


@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_the_mirror_with_the_tap_of_a_guided_run_fed_back(gpu, w, h):
    """SVGF's loop: the step's colour and variance go through `run_guided(levels=2, tap_level=1)`, whose tap is fed back."""
    from denoise_cases import synthetic

    dn = render.Denoiser(w, h)
    albedo = synthetic(w, h, 9 * w + h)[4]

    def tap_of(k, got, f):
        g = to_gbuffer(f["index"], f["normal"], f["point"], albedo)
        _, tap = dn.run_guided(torch.from_numpy(got[0]).cuda(), torch.from_numpy(got[1]).cuda(), g, levels=2, tap_level=1)
        torch.cuda.synchronize()
        return tap.cpu().numpy()

    for kind, frames in both_cameras(w, h):
        for prm in PARAMS:
            run_with_feedback(frames, w, h, f"{w}x{h} {kind} tap {prm}", tap_of, **prm)
    dn.close()


@pytest.mark.parametrize("w,h", SIZES)
def test_a_feedback_handle_without_feedback_is_a_moments_handle(gpu, w, h):
    for kind, frames in both_cameras(w, h):
        a, b = render.Temporal(w, h, moments=True, feedback=True), render.Temporal(w, h, moments=True)
        want = temporal_moments_ref.TemporalMoments(w, h)
        for k, f in enumerate(frames):
            x, y, z = gpu_step(a, *frame_args(f), 8), gpu_step(b, *frame_args(f), 8), want.step(*frame_args(f), 8)
            for name, p, q, r in zip(NAMES, x, y, z):
                same_bits(p, q, f"{w}x{h} {kind} step {k} {name}: feedback handle against moments handle")
                same_bits(p, r, f"{w}x{h} {kind} step {k} {name}: feedback handle against the moments mirror")
        a.close(), b.close()


def test_device_gives_the_hand_derived_answers(gpu):
    """Every case of tests/temporal_feedback_cases.py against its RATIONAL expectation directly — not through the mirror."""
    def step(tm, s):
        return gpu_step(tm, s.rgb, s.index, s.normal, s.point, s.camera, s.spp, **s.params)

    for c in cases.cases():
        h, w = c.steps[0].index.shape
        tm = render.Temporal(w, h, moments=True, feedback=True)
        out = c.run(tm, step, gpu_feedback)
        c.check(*out, "device")
        tm.close()


@pytest.mark.parametrize("w,h", [(45, 23), (97, 41)])
def test_the_tap_is_the_run_of_that_many_levels(gpu, w, h):
    """levels = 4, tap_level 1 .. 4, with the built-in choice of the levels' LDS form and with RAYZ_DEBUG_DENOISE_LDS_STRIDE 0 (every
    level direct) and 4 (strides 1, 2, 4 staged), so every level kernel is tapped as a level and as the last: the tap equals
    `run_guided(levels=t)`'s output bit for bit, and `out` and `var_out` equal the untapped run's — also with `out` in place."""
    from denoise_cases import synthetic
    from denoise_guided_cases import guided_variance

    rgb, index, normal, point, albedo = synthetic(w, h, 3 * w + h)
    var = guided_variance(rgb, 11)
    x, v, g = torch.from_numpy(rgb).cuda(), torch.from_numpy(var).cuda(), to_gbuffer(index, normal, point, albedo)
    dn = render.Denoiser(w, h)
    knob = capi.DEBUG_DENOISE_LDS_STRIDE
    try:
        for stride in (-1, 0, 4):
            render.debug_set(knob, stride)
            want_out, want_var = host(*dn.run_guided(x, v, g, var_out=True, levels=4))
            for t in (1, 2, 3, 4):
                want_tap, = host(dn.run_guided(x, v, g, levels=t))
                out, var_out, tap = host(*dn.run_guided(x, v, g, var_out=True, levels=4, tap_level=t))
                same_bits(tap, want_tap, f"{w}x{h} LDS stride {stride} tap {t}")
                same_bits(out, want_out, f"{w}x{h} LDS stride {stride} tap {t}: out")
                same_bits(var_out, want_var, f"{w}x{h} LDS stride {stride} tap {t}: var_out")
                y = x.clone()
                out, var_out, tap = host(*dn.run_guided(y, v, g, out=y, var_out=True, levels=4, tap_level=t))
                same_bits(tap, want_tap, f"{w}x{h} LDS stride {stride} tap {t}, in place")
                same_bits(out, want_out, f"{w}x{h} LDS stride {stride} tap {t}, in place: out")
                same_bits(var_out, want_var, f"{w}x{h} LDS stride {stride} tap {t}, in place: var_out")
            assert not np.array_equal(want_out, host(dn.run_guided(x, v, g, levels=1))[0])
    finally:
        render.debug_set(knob, -1)
    with pytest.raises(capi.RayzHipError, match="tap_level"):
        dn.run_guided(x, v, g, levels=4, tap_level=5)
    with pytest.raises(capi.RayzHipError, match="neither"):
        dn.run_guided(x, v, g, levels=4, tap_level=1, tap_out=x)
    with pytest.raises(ValueError, match="tap_level"):
        dn.run_guided(x, v, g, levels=4, tap_out=torch.empty_like(x))
    dn.close()


def test_the_state_rules(gpu):
    w, h = 33, 9
    f = temporal_cases.plane_sequence(w, h, 12, ORIGINS[:1])[0]
    x, v, g = torch.from_numpy(f["rgb"]).cuda(), torch.from_numpy(f["var"]).cuda(), to_gbuffer(f["index"], f["normal"], f["point"])
    cam = camera_desc(f["camera"])
    plain = render.Temporal(w, h)
    with pytest.raises(capi.RayzHipError, match="not in moments mode"):
        plain.track_feedback()
    with pytest.raises(capi.RayzHipError, match="does not track feedback"):
        plain.feedback(x)
    plain.close()
    with pytest.raises(ValueError, match="needs moments"):
        render.Temporal(w, h, feedback=True)
    tm = render.Temporal(w, h, moments=True)
    with pytest.raises(capi.RayzHipError, match="does not track feedback"):
        tm.feedback(x)
    tm.step_moments(x, g, cam, 8)
    with pytest.raises(capi.RayzHipError, match="has history"):
        tm.track_feedback()
    with pytest.raises(capi.RayzHipError, match="does not track feedback"):
        tm.feedback(x)
    tm.reset()
    tm.track_feedback()
    tm.track_feedback()  # a second call does nothing
    with pytest.raises(capi.RayzHipError, match="no history"):
        tm.feedback(x)  # before the first step
    tm.step_moments(x, g, cam, 8)
    tm.feedback(x)
    tm.track_feedback()  # .. with history too, once the handle tracks it
    tm.reset()
    with pytest.raises(capi.RayzHipError, match="no history"):
        tm.feedback(x)  # after a reset
    with pytest.raises(ValueError, match="rgb must be"):
        tm.feedback(torch.zeros((h, w), device="cuda"))
    with pytest.raises(capi.RayzHipError, match="moments mode"):
        tm.step(x, v, g, cam, 8)  # still a moments handle
    tm.close()


def test_a_feedback_and_a_moments_handle_interleaved_on_one_stream(gpu):
    """Steps and feedbacks of a feedback handle and steps of a moments handle alternating on one stream, nothing synchronised in
    between, give what each gives alone (its mirror); the time reported is the last step's, not the feedback's."""
    w, h = 97, 41
    frames = temporal_cases.plane_sequence(w, h, 4197, ORIGINS)
    fb, mom = render.Temporal(w, h, moments=True, feedback=True), render.Temporal(w, h, moments=True)
    want_f, want_m = ref.TemporalFeedback(w, h), temporal_moments_ref.TemporalMoments(w, h)
    images = [random_image(w, h, 7 + k) for k in range(len(frames))]
    inputs = [(torch.from_numpy(f["rgb"]).cuda(), to_gbuffer(f["index"], f["normal"], f["point"]), camera_desc(f["camera"]),
               torch.from_numpy(img).cuda()) for f, img in zip(frames, images)]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    keep = []
    for x, g, cam, img in inputs:
        rf = fb.step_moments(x, g, cam, 8, length=True, w2=True, stream=s.cuda_stream)
        fb.feedback(img, stream=s.cuda_stream)
        keep.append((rf, mom.step_moments(x, g, cam, 8, length=True, w2=True, stream=s.cuda_stream)))
    s.synchronize()
    assert fb.timing() > 0
    for k, (f, img, (rf, rm)) in enumerate(zip(frames, images, keep)):
        for name, x, y in zip(NAMES, rf, want_f.step(*frame_args(f), 8)):
            same_bits(x.cpu().numpy(), y, f"feedback handle step {k} {name}")
        want_f.feedback(img)
        for name, x, y in zip(NAMES, rm, want_m.step(*frame_args(f), 8)):
            same_bits(x.cpu().numpy(), y, f"moments handle step {k} {name}")
    fb.close(), mom.close()


def test_destroy_after_the_stream_with_a_feedback_pending(gpu):
    """A step and a feedback on a stream the caller then releases: the next step waits for the feedback through the handle's own
    event and sees it; and close() with a feedback pending on a released stream waits the same way."""
    w, h = 97, 41
    frames = temporal_cases.plane_sequence(w, h, 77, ORIGINS[:3])
    want = ref.TemporalFeedback(w, h)
    tm = render.Temporal(w, h, moments=True, feedback=True)
    tensors = [(torch.from_numpy(np.ascontiguousarray(f["rgb"])).cuda(), to_gbuffer(f["index"], f["normal"], f["point"])) for f in frames]
    images = [random_image(w, h, 3 + k) for k in range(3)]
    dimages = [torch.from_numpy(i).cuda() for i in images]
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    for k in range(2):
        tm.step_moments(tensors[k][0], tensors[k][1], camera_desc(frames[k]["camera"]), 8, stream=s.cuda_stream)
        tm.feedback(dimages[k], stream=s.cuda_stream)
    del s
    out = tm.step_moments(tensors[2][0], tensors[2][1], camera_desc(frames[2]["camera"]), 8, length=True, w2=True)
    torch.cuda.synchronize()
    for k, f in enumerate(frames):
        r = want.step(*frame_args(f), 8)
        want.feedback(images[k])
    for name, x, y in zip(NAMES, out, r):
        same_bits(x.cpu().numpy(), y, f"a step after feedbacks on a released stream: {name}")
    s = torch.cuda.Stream()
    tm.feedback(dimages[2], stream=s.cuda_stream)
    del s
    tm.close()  # (waits for that feedback through the handle's event)
    torch.cuda.synchronize()
