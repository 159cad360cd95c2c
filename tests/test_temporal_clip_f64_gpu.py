"""The float64 statement of DESIGN.md §4.28 (tests/temporal_clip_f64.py) on the GPU: the moments clip step of the device within
the derived bound on the moving sequence at (45, 23) and (97, 41), at the defaults and with the temporal estimate selected, and on
threeSpheres under the orbit with device G-buffers; at most 2 % of a step's hit pixels excluded; clipped and unclipped pixels with
history in every run; the plain clip step's colour and length equal to the moments step's bit for bit; and the sky pixels of an
ACCUMULATE handle within the bound on the moving sequence."""
import pytest
import torch

import temporal_cases
import temporal_clip_f64 as f64
from rayz_amd import render
from test_temporal_clip_gpu import moments_step, plain_step, sequences
from test_temporal_gpu import same_bits, three_spheres, tracked_frame

pytestmark = pytest.mark.gpu

PARAMS = {"defaults": {}, "w2_max 0.6": dict(w2_max=0.6)}


@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("w,h", [(45, 23), (97, 41)])
def test_device_within_the_f64_bound_under_a_moving_camera(gpu, w, h, pname):
    prm = PARAMS[pname]
    frames = sequences(w, h)["moving"]
    tm, pl, r = render.Temporal(w, h, moments=True, clip="variance"), render.Temporal(w, h, clip="variance"), f64.TemporalClipMomentsF64(w, h)
    tm.set_clip("variance", clipped=True)
    some = none = 0
    for k, f in enumerate(frames):
        want = r.step(f["rgb"], f["index"], f["normal"], f["point"], f["camera"], f["spp"], bound=True, **prm)
        got = moments_step(tm, f, **prm)
        hit = f["index"] >= 0
        ratios, shares = f64.within_bound(got, want, hit, f"moving {w}x{h} {pname} step {k}")
        cl = tm.clipped.cpu().numpy().astype(bool)
        found = hit & (got[2] > f["spp"])
        some, none = some + int(cl.sum()), none + int((found & ~cl).sum())
        print(f"moving {w}x{h} {pname} step {k}: |diff|/bound {ratios[0]:.3f} {ratios[1]:.3f} {ratios[2]:.3f} {ratios[3]:.3f}; excluded "
              f"{shares[0]:.4f} {shares[1]:.4f}; clipped {cl.sum() / max(found.sum(), 1):.3f} of the pixels with history")
        if pname == "defaults":  # §4.16 rule 1 carries the bound to the plain clip step
            other = plain_step(pl, f)
            same_bits(other[0], got[0], f"step {k}: the plain step's colour")
            same_bits(other[2], got[2], f"step {k}: the plain step's length")
    assert some and none, (some, none)
    tm.close(), pl.close()


@pytest.mark.parametrize("w,h", [(45, 23), (97, 41)])
def test_device_within_the_f64_bound_on_the_sky(gpu, w, h):
    """The background pixels of a handle in ACCUMULATE mode on the moving sequence, with the temporal estimate selected."""
    frames = sequences(w, h)["moving"]
    tm, r = render.Temporal(w, h, moments=True, background="accumulate", clip="variance"), f64.TemporalClipMomentsF64(w, h, background=True)
    tm.set_clip("variance", clipped=True)
    some = none = 0
    for k, f in enumerate(frames):
        want = r.step(f["rgb"], f["index"], f["normal"], f["point"], f["camera"], f["spp"], bound=True, w2_max=0.6)
        got = moments_step(tm, f, w2_max=0.6)
        bg = f["index"] < 0
        ratios, shares = f64.within_bound(got, want, bg, f"sky moving {w}x{h} step {k}")
        cl, found = tm.clipped.cpu().numpy().astype(bool) & bg, bg & (got[2] > f["spp"])
        some, none = some + int(cl.sum()), none + int((found & ~cl).sum())
        print(f"sky moving {w}x{h} step {k}: |diff|/bound {ratios[0]:.3f} {ratios[1]:.3f} {ratios[2]:.3f} {ratios[3]:.3f}; excluded {shares[0]:.4f} "
              f"{shares[1]:.4f}; clipped {cl.sum() / max(found.sum(), 1):.3f} of the sky pixels with history")
    assert some and none, (some, none)
    tm.close()


def test_device_within_the_f64_bound_under_an_orbit(gpu, oracle):
    """threeSpheres at 64x36 through `temporal_cases.orbit_views`: G-buffers from `DeviceScene.gbuffer`, frames of 8 spp from tracked
    progressive handles, one seed per frame; the device's moments clip step against the f64 reference fed the same device arrays.
    w2_max = 0.3: off the values 1/2, 1/3, 1/4, 1/5 that equal frames land on exactly (the default 1/4 puts every pixel of the
    fourth frame on the border of W2 > w2_max), as tests/test_temporal_moments_f64_gpu.py's orbit chooses its own."""
    t, sd, cam, p = three_spheres(8, 4)
    w, h = p.width, p.height
    ds = render.DeviceScene(sd)
    tm, r = render.Temporal(w, h, moments=True, clip="variance"), f64.TemporalClipMomentsF64(w, h)
    tm.set_clip("variance", clipped=True)
    some = none = 0
    for k, view in enumerate(temporal_cases.orbit_views()):
        c = temporal_cases.orbit_camera(oracle, view, w, h)
        frame, _ = tracked_frame(ds, c, p, 100 + k)
        g = ds.gbuffer(c, p)
        ds.query_sync()
        out = tm.step_moments(frame, g, c, 8, length=True, w2=True, w2_max=0.3)
        torch.cuda.synchronize()
        got = tuple(x.cpu().numpy() for x in out)
        rgb, idx, nrm, pt = (x.cpu().numpy() for x in (frame, g.index, g.normal, g.point))
        want = r.step(rgb, idx, nrm, pt, c, 8, bound=True, w2_max=0.3)
        hit = idx >= 0
        ratios, shares = f64.within_bound(got, want, hit, f"orbit step {k}")
        cl = tm.clipped.cpu().numpy().astype(bool)
        found = hit & (got[2] > 8)
        some, none = some + int(cl.sum()), none + int((found & ~cl).sum())
        print(f"orbit step {k}: |diff|/bound {ratios[0]:.3f} {ratios[1]:.3f} {ratios[2]:.3f} {ratios[3]:.3f}; excluded {shares[0]:.4f} "
              f"{shares[1]:.4f}; clipped {cl.sum() / max(found.sum(), 1):.3f} of the pixels with history")
    assert some and none, (some, none)
    tm.close(), ds.close()
