"""Temporal accumulation's background mode on the GPU (rayz_hip_temporal_set_background, `render.Temporal(background=...)`;
DESIGN.md §4.27): every output of every step — plain, moments and both counts steps, with the mode switched mid-sequence — equals
the CPU restatement (tests/temporal_background_mirror.cpp) bit for bit; the hand-derived answers of
tests/temporal_background_cases.py; the f64 statement's bound; a still camera's two-frame mean on a traced scene; a lattice cycle
that ends in the whole frame's step at EVERY pixel; what the mode refuses; and a handle in the default mode unchanged."""
import numpy as np
import pytest
import torch

import temporal_background_cases as cases
import temporal_background_f64 as f64
import temporal_background_ref as ref
import temporal_cases
import temporal_ref
from rayz_amd import capi, render
from test_temporal_counts_gpu import lattice_phase
from test_temporal_gpu import SIZES, camera_desc, same_bits, three_spheres, to_gbuffer, tracked_frame

pytestmark = pytest.mark.gpu

BINDING = dict(alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)
DRAW = np.array([0, 0, 1, 4, 8])
NAN = np.float32(np.nan)


def sequences(w, h):
    out = {"general": temporal_cases.general_sequence(w, h, 5 * w + h), "edge": temporal_cases.edge_sequence(w, h, 7 * w + h),
           "moving": temporal_cases.moving_sequence(w, h, 3 * w + h)}
    return {k: [dict(f, spp=f.get("spp", 8)) for f in v] for k, v in out.items()}


def sparse(frames, seed):
    """The frames with per-pixel counts drawn from {0, 0, 1, 4, 8} for spp and NaN colour and variance wherever the count is 0."""
    rng = np.random.default_rng(seed)
    out = []
    for f in frames:
        counts = rng.choice(DRAW, size=f["index"].shape).astype(np.int32)
        rgb, var = f["rgb"].copy(), f["var"].copy()
        rgb[counts == 0] = NAN
        var[counts == 0] = NAN
        out.append(dict(f, rgb=rgb, var=var, spp=counts))
    return out


def _spp(spp):
    return int(spp) if np.isscalar(spp) else torch.from_numpy(np.ascontiguousarray(spp, dtype=np.int32)).cuda()


def plain_step(tm, f, **prm):
    x, v = torch.from_numpy(f["rgb"]).cuda(), torch.from_numpy(f["var"]).cuda()
    res = tm.step(x, v, to_gbuffer(f["index"], f["normal"], f["point"]), camera_desc(f["camera"]), _spp(f["spp"]), length=True, **prm)
    torch.cuda.synchronize()
    return tuple(r.cpu().numpy() for r in res)


def moments_step(tm, f, **prm):
    x = torch.from_numpy(f["rgb"]).cuda()
    res = tm.step_moments(x, to_gbuffer(f["index"], f["normal"], f["point"]), camera_desc(f["camera"]), _spp(f["spp"]), length=True, w2=True,
                          **prm)
    torch.cuda.synchronize()
    return tuple(r.cpu().numpy() for r in res)


def mirror_step(m, f, **prm):
    if isinstance(m, ref.Temporal):
        return m.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], f["spp"], **prm)
    return m.step(f["rgb"], f["index"], f["normal"], f["point"], f["camera"], f["spp"], **prm)


def run(frames, w, h, moments, modes, what, **prm):
    """The frames through the mirror and a device handle, step k in modes[k]; the handle's taken bytes stay 0."""
    mirror = (ref.TemporalMoments if moments else ref.Temporal)(w, h)
    tm = render.Temporal(w, h, moments=moments)
    tm.set_resampling("bilinear", taken=True)
    blended = 0
    for k, (f, mode) in enumerate(zip(frames, modes)):
        mirror.set_background(mode)
        tm.set_background(mode)
        assert tm.background == mode
        want = mirror_step(mirror, f, **prm)
        got = (moments_step if moments else plain_step)(tm, f, **prm)
        for name, x, y in zip(("colour", "variance", "length", "W2"), got, want):
            same_bits(x, y, f"{what} step {k} ({mode}) {name}")
        assert not tm.taken.any(), f"{what} step {k}: taken bytes"
        if mode == "accumulate":
            bg = f["index"] < 0
            blended += int((want[2][bg] > (f["spp"] if np.isscalar(f["spp"]) else f["spp"][bg])).sum())  # a length beyond its own count
    tm.close()
    return blended


@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_the_mirror(gpu, w, h):
    """The general, the edge and the moving sequence through the plain and the moments handle, with one spp and with counts drawn
    per pixel (NaN inputs where the count is 0): INPUT for the first step and ACCUMULATE from then on — the static and the moving
    kernels read what an INPUT step left — and ACCUMULATE until an INPUT step ends the sequence.  At the defaults; the plain steps
    with every parameter binding as well."""
    for name, frames in sequences(w, h).items():
        n = len(frames)
        for moments in (False, True):
            for fs, kind in ((frames, "spp"), (sparse(frames, 3 * w + h), "counts")):
                what = f"{w}x{h} {name} moments={moments} {kind}"
                blended = run(fs, w, h, moments, ["input"] + ["accumulate"] * (n - 1), what)
                run(fs, w, h, moments, ["accumulate"] * (n - 1) + ["input"], what + " then input")
                if w * h > 100:
                    assert blended > 0, f"{what}: no background pixel found history"
        run(frames, w, h, False, ["input"] + ["accumulate"] * (n - 1), f"{w}x{h} {name} binding", **BINDING)
        run(frames, w, h, True, ["input"] + ["accumulate"] * (n - 1), f"{w}x{h} {name} w2_max 1", w2_max=1.0)


def test_device_gives_the_hand_derived_answers(gpu):
    """Every case of tests/temporal_background_cases.py against its RATIONAL expectation directly — not through the mirror."""
    def step(moments):
        def fn(tm, s):
            tm.set_background(s.mode)
            f = dict(rgb=s.rgb, var=s.var, index=s.index, normal=s.normal, point=s.point, camera=s.camera, spp=cases.counts_of(s))
            return (moments_step if moments else plain_step)(tm, f, **s.params)
        return fn

    for moments, cs in ((False, cases.cases()), (True, cases.moments_cases())):
        for c in cs:
            h, w = c.steps[0].index.shape
            tm = render.Temporal(w, h, moments=moments)
            c.check(*c.run(tm, step(moments)), "device")
            tm.close()


def lowered(view):
    """A view of `temporal_cases.orbit_views` brought down to the spheres' height and raised a little: threeSpheres' own views look
    down at the ground and see no sky; these see it in about four pixels of ten, above the ground and behind the spheres."""
    (fx, fy, fz), (ax, ay, az) = view
    return (fx, fy - 1.5, fz), (ax, ay + 0.3, az)


@pytest.mark.parametrize("pname", ["defaults", "binding"])
@pytest.mark.parametrize("w,h", [(45, 23), (97, 41)])
def test_device_within_the_f64_bound_under_a_moving_camera(gpu, w, h, pname):
    """moving_sequence in ACCUMULATE mode against tests/temporal_background_f64.py: every background value within the bound, at most
    2 % of the background excluded, and behind the first step more than half of the background finds history."""
    prm = {} if pname == "defaults" else BINDING
    frames = sequences(w, h)["moving"]
    tm, r = render.Temporal(w, h, background="accumulate"), f64.TemporalBackgroundF64(w, h)
    for k, f in enumerate(frames):
        want = r.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], f["spp"], bound=True, **prm)
        got = plain_step(tm, f, **prm)
        bg = f["index"] < 0
        ratios, share = f64.within_bound(got, want, bg, f"moving {w}x{h} {pname} step {k}")
        found = float((got[2][bg] > f["spp"]).mean())
        print(f"moving {w}x{h} {pname} step {k}: |diff|/bound {ratios[0]:.3f} {ratios[1]:.3f} {ratios[2]:.3f}; excluded {share:.4f}; "
              f"history found {found:.3f}")
        assert found == 0 if k == 0 else found > 0.5, (k, found)
    tm.close()


@pytest.mark.parametrize("views", ["orbit", "lowered"])
def test_device_within_the_f64_bound_under_an_orbit(gpu, oracle, views):
    """threeSpheres at 64x36 through `temporal_cases.orbit_views` — which see no sky: the bound then holds nothing but that no
    background appears — and through the same views lowered until they do: G-buffers from `DeviceScene.gbuffer`, frames of 8 spp in
    two chunks and their `noise_rgb()` from tracked progressive handles, one seed per frame; the device's ACCUMULATE step against
    the f64 reference fed the same device arrays."""
    t, sd, cam, p = three_spheres(8, 4)
    w, h = p.width, p.height
    ds = render.DeviceScene(sd)
    tm, r = render.Temporal(w, h, background="accumulate"), f64.TemporalBackgroundF64(w, h)
    for k, view in enumerate(temporal_cases.orbit_views()):
        c = temporal_cases.orbit_camera(oracle, lowered(view) if views == "lowered" else view, w, h)
        frame, var = tracked_frame(ds, c, p, 100 + k)
        g = ds.gbuffer(c, p)
        ds.query_sync()
        out = tm.step(frame, var, g, c, 8, length=True)
        torch.cuda.synchronize()
        got = tuple(x.cpu().numpy() for x in out)
        rgb, v, idx, nrm, pt = (x.cpu().numpy() for x in (frame, var, g.index, g.normal, g.point))
        want = r.step(rgb, v, idx, nrm, pt, c, 8, bound=True)
        bg = idx < 0
        ratios, share = f64.within_bound(got, want, bg, f"{views} step {k}")
        found = float((got[2][bg] > 8).mean()) if bg.any() else 0.0
        print(f"{views} step {k}: background {bg.mean():.3f}; |diff|/bound {ratios[0]:.3f} {ratios[1]:.3f} {ratios[2]:.3f}; "
              f"excluded {share:.4f}; history found {found:.3f}")
        if views == "lowered":
            assert 0.1 < bg.mean() < 0.9 and (found > 0.5 if k else found == 0), (k, bg.mean(), found)
    tm.close(), ds.close()


def sky_scene(oracle):
    """threeSpheres at 64x36, 8 spp in two chunks, through the first lowered view: (device scene, camera, params, its G-buffer)."""
    t, sd, _, p = three_spheres(8, 4)
    cam = temporal_cases.orbit_camera(oracle, lowered(temporal_cases.orbit_views()[0]), p.width, p.height)
    ds = render.DeviceScene(sd)
    g = ds.gbuffer(cam, p)
    ds.query_sync()
    return ds, cam, p, g


def test_a_still_cameras_background_is_the_two_frame_mean(gpu, oracle):
    """threeSpheres at 64x36 with a still camera that sees sky, alpha_min = 0, n_max = inf, two tracked frames of different seeds:
    every background pixel's output is fma(1/2, c2 - c1, c1) bit for bit, its length 16; in INPUT mode it is c2."""
    ds, cam, p, g = sky_scene(oracle)
    w, h = p.width, p.height
    bg = (g.index < 0).cpu().numpy()
    assert 0.1 < bg.mean() < 0.9
    (c1, v1), (c2, v2) = tracked_frame(ds, cam, p, 41), tracked_frame(ds, cam, p, 97)
    a, b = render.Temporal(w, h, background="accumulate"), render.Temporal(w, h)
    prm = dict(alpha_min=0.0, n_max=float("inf"))
    for tm in (a, b):
        tm.step(c1, v1, g, cam, 8, **prm)
    ra, rb = a.step(c2, v2, g, cam, 8, length=True, **prm), b.step(c2, v2, g, cam, 8, length=True, **prm)
    torch.cuda.synchronize()
    h1, h2 = c1.cpu().numpy(), c2.cpu().numpy()
    want = (h1.astype(np.float64) + 0.5 * (h2 - h1).astype(np.float64)).astype(np.float32)  # (one rounding: the halving is exact)
    assert (h1[bg] != h2[bg]).any()
    same_bits(ra[0].cpu().numpy()[bg], want[bg], "accumulate: the background's mean")
    assert (ra[2].cpu().numpy()[bg] == 16).all()
    same_bits(rb[0].cpu().numpy()[bg], h2[bg], "input: the background's input")
    for x, y in zip(ra, rb):
        same_bits(x.cpu().numpy()[~bg], y.cpu().numpy()[~bg], "hit pixels in both modes")
    a.close(), b.close(), ds.close()


def test_a_phase_cycle_ends_in_the_whole_frames_step_at_every_pixel(gpu, oracle):
    """threeSpheres at 64x36, 8 spp in two chunks, a still camera that sees sky, ACCUMULATE.  The four phases of an every-2nd-pixel lattice are traced
    sparsely into NaN-filled frames and stepped with their counts; after a cycle the output, the variance and the length — the
    records the step leaves — equal ONE scalar step of the whole tracked frame at EVERY pixel, the background included, and after a
    second cycle from another seed the second whole-frame step."""
    f = 2
    ds, cam, p, g = sky_scene(oracle)
    w, h = p.width, p.height
    assert 0.1 < (g.index < 0).float().mean() < 0.9
    whole, cycled = render.Temporal(w, h, background="accumulate"), render.Temporal(w, h, background="accumulate")
    for cycle, seed in enumerate((41, 97)):
        frame, var = tracked_frame(ds, cam, p, seed)
        want = whole.step(frame, var, g, cam, 8, length=True)
        for phase in render.phase_sequence(f):
            x, v, counts = lattice_phase(ds, cam, p, seed, f, phase, True)
            got = cycled.step(x, v, g, cam, counts, length=True)
        torch.cuda.synchronize()
        for name, a, b in zip(("colour", "variance", "length"), got, want):
            same_bits(a.cpu().numpy(), b.cpu().numpy(), f"cycle {cycle} {name}")
        assert (want[2].cpu().numpy() == 8 * (cycle + 1)).all()
    whole.close(), cycled.close(), ds.close()


def test_refusals(gpu):
    """The mode value is checked before the handle; feedback and cubic handles refuse the mode, and the mode refuses them."""
    lib = capi.load()
    assert lib.rayz_hip_temporal_set_background(None, 2) == capi.ERR_BAD_ARG and b"background mode" in lib.rayz_hip_last_error()
    assert lib.rayz_hip_temporal_set_background(None, capi.TEMPORAL_BACKGROUND_ACCUMULATE) == capi.ERR_STATE
    assert lib.rayz_hip_temporal_get_background(None, None) == capi.ERR_STATE
    w, h = 33, 9
    state = rf"status {capi.ERR_STATE}\)"
    fb = render.Temporal(w, h, moments=True, feedback=True)
    with pytest.raises(capi.RayzHipError, match=state + ".*feedback"):
        fb.set_background("accumulate")
    assert fb.background == "input"
    fb.close()
    mm = render.Temporal(w, h, moments=True, background="accumulate")
    with pytest.raises(capi.RayzHipError, match=state + ".*background"):
        mm.track_feedback()
    with pytest.raises(capi.RayzHipError, match=state + ".*background"):
        mm.set_resampling("cubic")
    assert mm.background == "accumulate" and mm.resampling == "bilinear"
    mm.set_background("input")
    mm.set_resampling("cubic")
    with pytest.raises(capi.RayzHipError, match=state + ".*cubic"):
        mm.set_background("accumulate")
    assert mm.background == "input"
    with pytest.raises(capi.RayzHipError, match=rf"status {capi.ERR_BAD_ARG}\)"):
        capi.check(lib, lib.rayz_hip_temporal_set_background(mm._h, 7), "rayz_hip_temporal_set_background")
    mm.close()
    with pytest.raises(ValueError, match="background must be one of"):
        render.Temporal(w, h, background="sky")
    for bad in (dict(moments=True, feedback=True), dict(resampling="cubic")):
        with pytest.raises(ValueError, match="accumulate"):
            render.Temporal(w, h, background="accumulate", **bad)
    tm = render.Temporal(w, h)
    with pytest.raises(ValueError, match="background must be one of"):
        tm.set_background("sky")
    tm.close()


def test_the_default_mode_is_unchanged(gpu):
    """A handle asked for its mode, set to "input", to "accumulate" and back before and between its steps gives the bits of
    tests/temporal_mirror.cpp — the steps as they were — and of a handle that was never asked."""
    w, h = 97, 41
    frames = sequences(w, h)["moving"]
    mirror = temporal_ref.Temporal(w, h)
    a, b = render.Temporal(w, h), render.Temporal(w, h)
    for k, f in enumerate(frames):
        assert b.background == "input"
        b.set_background("input")
        b.set_background("accumulate")
        b.set_background("input")
        want = mirror.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], f["spp"])
        for tm in (a, b):
            for name, x, y in zip(("colour", "variance", "length"), plain_step(tm, f), want):
                same_bits(x, y, f"step {k} {name}")
    a.close(), b.close()
