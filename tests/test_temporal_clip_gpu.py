"""Temporal accumulation's clip mode on the GPU (rayz_hip_temporal_set_clip, `render.Temporal(clip=...)`): the
hand-derived answers of tests/temporal_clip_cases.py; every output and the clipped bytes of every step — plain and moments, both
background modes, the clip's parameters at their defaults and at their ends, the mode switched mid-sequence — equal to the CPU
restatement (tests/temporal_clip_mirror.cpp) bit for bit; a VARIANCE handle's first and static steps equal to an OFF handle's;
what the mode refuses; and a handle in the default mode unchanged."""
import ctypes as C

import numpy as np
import pytest
import torch

import temporal_cases
import temporal_clip_cases as cases
import temporal_clip_ref as ref
import temporal_ref
from rayz_amd import capi, render
from test_temporal_gpu import SIZES, camera_desc, same_bits, to_gbuffer

pytestmark = pytest.mark.gpu

INF = float("inf")
BINDING = dict(alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)
# the defaults; gamma at 0, 1/2 and +inf; min_taps at its ends
CLIPS = [dict(), dict(gamma=0.0), dict(gamma=0.5), dict(gamma=INF), dict(min_taps=2.0), dict(min_taps=49.0)]


def sequences(w, h):
    out = {"general": temporal_cases.general_sequence(w, h, 5 * w + h), "edge": temporal_cases.edge_sequence(w, h, 7 * w + h),
           "moving": temporal_cases.moving_sequence(w, h, 3 * w + h)}
    return {k: [dict(f, spp=f.get("spp", 8)) for f in v] for k, v in out.items()}


def plain_step(tm, f, **prm):
    x, v = torch.from_numpy(f["rgb"]).cuda(), torch.from_numpy(f["var"]).cuda()
    res = tm.step(x, v, to_gbuffer(f["index"], f["normal"], f["point"]), camera_desc(f["camera"]), int(f["spp"]), length=True, **prm)
    torch.cuda.synchronize()
    return tuple(r.cpu().numpy() for r in res)


def moments_step(tm, f, **prm):
    x = torch.from_numpy(f["rgb"]).cuda()
    res = tm.step_moments(x, to_gbuffer(f["index"], f["normal"], f["point"]), camera_desc(f["camera"]), int(f["spp"]), length=True, w2=True,
                          **prm)
    torch.cuda.synchronize()
    return tuple(r.cpu().numpy() for r in res)


def mirror_step(m, f, **prm):
    if isinstance(m, ref.Temporal):
        return m.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], f["spp"], **prm)
    return m.step(f["rgb"], f["index"], f["normal"], f["point"], f["camera"], f["spp"], **prm)


def run(frames, w, h, moments, background, clips, what, **prm):
    """The frames through the mirror and a device handle, step k with the clip clips[k] ((mode, gamma, min_taps)): every output and
    the clipped bytes.  Returns (clipped pixels, pixels with history that were not clipped) over the steps."""
    mirror = (ref.TemporalMoments if moments else ref.Temporal)(w, h, background)
    tm = render.Temporal(w, h, moments=moments, background=background)
    keep = torch.full((h, w), 7, dtype=torch.uint8, device="cuda")
    some = none = 0
    for k, (f, (mode, gamma, taps)) in enumerate(zip(frames, clips)):
        mirror.set_clip(mode, gamma, taps)
        tm.set_clip(mode, gamma, taps, clipped=keep)
        assert tm.clip == mode and tm.clipped is keep
        want = mirror_step(mirror, f, **prm)
        got = (moments_step if moments else plain_step)(tm, f, **prm)
        for name, x, y in zip(("colour", "variance", "length", "W2"), got, want):
            same_bits(x, y, f"{what} step {k} ({mode}) {name}")
        got_map = keep.cpu().numpy()
        assert (got_map == mirror.clipped).all(), f"{what} step {k} ({mode}): clipped bytes differ at {np.argwhere(got_map != mirror.clipped)[:4].tolist()}"
        if k == 0 or mirror.last_static or mode == "off":
            assert not got_map.any(), f"{what} step {k}: a step that clips nothing left bytes set"
        some, none = some + int(got_map.sum()), none + int(((want[2] > f["spp"]) & (got_map == 0)).sum())
    tm.close()
    return some, none


@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_the_mirror(gpu, w, h):
    """The general, the edge and the moving sequence through the plain and the moments handle, with the background passed through
    and accumulated, in VARIANCE mode at the defaults, with gamma 0, 1/2 and +inf and with min_taps 2 and 49; the plain and the
    moments step with every parameter binding as well.  At the defaults, frames larger than the halo clip some pixels with history
    and leave others."""
    for name, frames in sequences(w, h).items():
        n = len(frames)
        for moments in (False, True):
            for background in ("input", "accumulate"):
                for c in CLIPS:
                    clip = ("variance", c.get("gamma"), c.get("min_taps"))
                    what = f"{w}x{h} {name} moments={moments} {background} {c}"
                    some, none = run(frames, w, h, moments, background, [clip] * n, what)
                    if not c and w * h > 1000:
                        assert some and none, (what, some, none)
                    if c.get("gamma") == INF:
                        assert not some, what
            run(frames, w, h, moments, "accumulate", [("variance", None, None)] * n, f"{w}x{h} {name} moments={moments} binding", **BINDING)
        run(frames, w, h, True, "input", [("variance", None, None)] * n, f"{w}x{h} {name} w2_max 1", w2_max=1.0)


@pytest.mark.parametrize("moments", [False, True])
def test_the_mode_switches_mid_sequence(gpu, moments):
    """OFF, VARIANCE, VARIANCE with other parameters, OFF, VARIANCE over the moving sequence: the mode is no state of the history, and
    an OFF step clears the bytes the step before it set."""
    w, h = 97, 41
    frames = sequences(w, h)["moving"]
    clips = [("off", None, None), ("variance", None, None), ("variance", 0.25, 9.0), ("off", 0.25, 9.0), ("variance", 2.0, 2.0)]
    assert len(frames) >= 4
    some, _ = run(frames, w, h, moments, "accumulate", clips[:len(frames)], f"switching moments={moments}")
    assert some


def test_device_gives_the_hand_derived_answers(gpu):
    """Every case of tests/temporal_clip_cases.py against its RATIONAL expectation directly — not through the mirror —, with the
    clipped bytes of its last step."""
    def step(moments):
        def fn(tm, s):
            tm.set_background(s.mode)
            tm.set_clip(s.clip, s.gamma, s.min_taps, clipped=tm.clipped if tm.clipped is not None else True)
            f = dict(rgb=s.rgb, var=s.var, index=s.index, normal=s.normal, point=s.point, camera=s.camera, spp=s.spp)
            return (moments_step if moments else plain_step)(tm, f, **s.params)
        return fn

    for moments, cs in ((False, cases.cases()), (True, cases.moments_cases())):
        for c in cs:
            h, w = c.steps[0].index.shape
            tm = render.Temporal(w, h, moments=moments)
            c.check(*c.run(tm, step(moments)), "device")
            got = tm.clipped.cpu().numpy()
            for p, want in c.clipped.items():
                assert got[p] == want, (c.name, p, got[p], want)
            tm.close()


@pytest.mark.parametrize("moments", [False, True])
def test_first_and_static_steps_are_the_off_steps(gpu, moments):
    """A VARIANCE handle and an OFF handle fed the general sequence — a first frame, a static step, then a move — and then the first
    frame again after reset(): the first and the static step, and the first step after the reset, agree bit for bit and leave the
    bytes 0; the moving step clips."""
    w, h = 97, 41
    frames = sequences(w, h)["general"]
    step = moments_step if moments else plain_step
    a, b = render.Temporal(w, h, moments=moments, clip="variance"), render.Temporal(w, h, moments=moments)
    a.set_clip("variance", clipped=True)
    assert (a.clip, b.clip) == ("variance", "off") and a.clip_params == capi.TEMPORAL_CLIP_DEFAULTS == b.clip_params
    for k, f in enumerate(frames[:2]):
        for name, x, y in zip(("colour", "variance", "length", "W2"), step(a, f), step(b, f)):
            same_bits(x, y, f"step {k} {name}")
        assert not a.clipped.any()
    step(a, frames[2])
    assert a.clipped.any()
    a.reset(), b.reset()
    for name, x, y in zip(("colour", "variance", "length", "W2"), step(a, frames[0]), step(b, frames[0])):
        same_bits(x, y, f"after reset {name}")
    assert not a.clipped.any()
    a.close(), b.close()


def test_refusals(gpu):
    """The arguments are checked before the handle; feedback and cubic handles refuse the mode and the mode refuses them; a VARIANCE
    handle takes no counts step; a step refuses bytes that are one of its outputs or the taken bytes."""
    lib = capi.load()
    assert lib.rayz_hip_temporal_set_clip(None, 2, None, None) == capi.ERR_BAD_ARG and b"clip mode" in lib.rayz_hip_last_error()
    assert lib.rayz_hip_temporal_set_clip(None, capi.TEMPORAL_CLIP_VARIANCE, None, None) == capi.ERR_STATE
    w, h = 33, 9
    state, bad_arg = rf"status {capi.ERR_STATE}\)", rf"status {capi.ERR_BAD_ARG}\)"
    fb = render.Temporal(w, h, moments=True, feedback=True)
    with pytest.raises(capi.RayzHipError, match=state + ".*feedback"):
        fb.set_clip("variance")
    assert fb.clip == "off"
    fb.close()
    cu = render.Temporal(w, h, resampling="cubic")
    with pytest.raises(capi.RayzHipError, match=state + ".*cubic"):
        cu.set_clip("variance")
    cu.set_clip("off", gamma=2.0)  # (OFF is taken by every handle, with its parameters)
    assert cu.clip == "off" and cu.clip_params == {"gamma": 2.0, "min_taps": 4.0}
    cu.close()
    mm = render.Temporal(w, h, moments=True, clip="variance", clip_gamma=0.5, clip_min_taps=9)
    assert mm.clip == "variance" and mm.clip_params == {"gamma": 0.5, "min_taps": 9.0}
    with pytest.raises(capi.RayzHipError, match=state + ".*clip"):
        mm.track_feedback()
    with pytest.raises(capi.RayzHipError, match=state + ".*clip"):
        mm.set_resampling("cubic")
    assert mm.resampling == "bilinear"
    for gamma, taps in ((-1.0, 4.0), (float("nan"), 4.0), (1.0, 1.0), (1.0, 50.0)):
        with pytest.raises(capi.RayzHipError, match=bad_arg):
            mm.set_clip("variance", gamma, taps)
    assert mm.clip_params == {"gamma": 0.5, "min_taps": 9.0}
    with pytest.raises(capi.RayzHipError, match=bad_arg):
        capi.check(lib, lib.rayz_hip_temporal_set_clip(mm._h, 7, None, None), "rayz_hip_temporal_set_clip")
    f = sequences(w, h)["moving"][0]
    counts = torch.ones((h, w), dtype=torch.int32, device="cuda")
    g, cam, x = to_gbuffer(f["index"], f["normal"], f["point"]), camera_desc(f["camera"]), torch.from_numpy(f["rgb"]).cuda()
    with pytest.raises(ValueError, match="variance"):
        mm.step_moments(x, g, cam, counts)
    out, vout = torch.empty_like(x), torch.empty_like(x)
    o = render._gbuffer_pointers(g, ["index", "normal", "point"])
    rc = lib.rayz_hip_temporal_step_moments_counts(mm._h, None, None, C.byref(cam), C.c_void_p(counts.data_ptr()), C.c_void_p(x.data_ptr()),
                                                   C.byref(o), C.c_void_p(out.data_ptr()), C.c_void_p(vout.data_ptr()), None, None, None)
    assert rc == capi.ERR_STATE and b"clip" in lib.rayz_hip_last_error()
    mm.close()
    pl = render.Temporal(w, h, clip="variance")
    v = torch.from_numpy(f["var"]).cuda()
    rc = lib.rayz_hip_temporal_step_counts(pl._h, None, C.byref(cam), C.c_void_p(counts.data_ptr()), C.c_void_p(x.data_ptr()),
                                           C.c_void_p(v.data_ptr()), C.byref(o), C.c_void_p(out.data_ptr()), C.c_void_p(vout.data_ptr()), None, None)
    assert rc == capi.ERR_STATE and b"clip" in lib.rayz_hip_last_error()
    # bytes that alias an output of the step, or the taken bytes
    length = torch.empty((h, w), dtype=torch.float32, device="cuda")
    pl.set_clip("variance", clipped=length.view(torch.uint8).reshape(-1)[:h * w].reshape(h, w))
    with pytest.raises(capi.RayzHipError, match=bad_arg + ".*d_clipped"):
        pl.step(x, v, g, cam, 8, length=length)
    both = torch.empty((h, w), dtype=torch.uint8, device="cuda")
    pl.set_resampling("bilinear", taken=both)
    pl.set_clip("variance", clipped=both)
    with pytest.raises(capi.RayzHipError, match=bad_arg + ".*d_clipped"):
        pl.step(x, v, g, cam, 8)
    pl.set_clip("variance", clipped=True)
    pl.step(x, v, g, cam, 8)
    torch.cuda.synchronize()
    assert not pl.clipped.any() and not pl.taken.any()
    pl.close()
    with pytest.raises(ValueError, match="clip must be one of"):
        render.Temporal(w, h, clip="box")
    tm = render.Temporal(w, h)
    with pytest.raises(ValueError, match="clip must be one of"):
        tm.set_clip("box")
    tm.close()


def test_the_default_mode_is_unchanged(gpu):
    """A handle asked for its mode, set to "off" with other parameters, to "variance" and back before and between its steps gives the
    bits of tests/temporal_mirror.cpp — the steps as they were."""
    w, h = 97, 41
    frames = sequences(w, h)["moving"]
    mirror = temporal_ref.Temporal(w, h)
    a, b = render.Temporal(w, h), render.Temporal(w, h)
    for k, f in enumerate(frames):
        assert b.clip == "off"
        b.set_clip("variance", 0.5)
        b.set_clip("off", 0.5, clipped=True)
        want = mirror.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], f["spp"])
        for tm in (a, b):
            for name, x, y in zip(("colour", "variance", "length"), plain_step(tm, f), want):
                same_bits(x, y, f"step {k} {name}")
        assert not b.clipped.any()
    a.close(), b.close()
