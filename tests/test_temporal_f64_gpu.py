"""Temporal accumulation on the GPU against the f64 statement of its contract DIRECTLY (tests/temporal_f64.py) —
not through the CPU mirror the kernel was written beside: every colour, variance and length of every step of `render.Temporal`
lies within the reference's derived bound, with at most 2 % of a step's hit pixels excluded, on a sequence that moves and turns a
general camera over two depth layers with unequal spp, and on device G-buffers and tracked progressive frames of threeSpheres under
a camera that orbits and dollies.  tests/test_temporal_f64_cpu.py runs the same sequences and the same orbit on the mirror."""
import functools

import numpy as np
import pytest
import torch

import temporal_cases
import temporal_f64
from rayz_amd import render
from test_temporal_gpu import frame_args, gpu_step, three_spheres, tracked_frame

pytestmark = pytest.mark.gpu

PARAMS = {"defaults": {}, "binding": dict(alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)}


@functools.lru_cache(maxsize=None)
def reference(w, h, pname, reset):
    """(frames, the f64 reference's per-step results with bound and mask) of moving_sequence; computed once, never changed."""
    frames = temporal_cases.moving_sequence(w, h, 5 * w + h)
    r = temporal_f64.TemporalF64(w, h)
    out = []
    for k, f in enumerate(frames):
        if reset and k == len(frames) - 1:
            r.reset()
        out.append(r.step(*frame_args(f), f["spp"], bound=True, **PARAMS[pname]))
    return frames, out


def without_length(ref):
    return ref[:2] + (ref[3][:2], ref[4])


@pytest.mark.parametrize("reset", [False, True], ids=["straight", "reset-before-last"])
@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("w,h", [(45, 23), (97, 41)])
def test_device_within_the_f64_bound_under_a_moving_camera(gpu, w, h, pname, reset):
    """Two device handles — out of place with the length, in place without it — through first, static, moved, turned and moved
    again at spp 4, 8, 16, 8, 4; neither size is a multiple of the 32x8 tile."""
    frames, ref = reference(w, h, pname, reset)
    a, b = render.Temporal(w, h), render.Temporal(w, h)
    for k, (f, r) in enumerate(zip(frames, ref)):
        if reset and k == len(frames) - 1:
            a.reset(), b.reset()
        hit = f["index"] >= 0
        what = f"moving {w}x{h} {pname} step {k}"
        got = gpu_step(a, *frame_args(f), f["spp"], **PARAMS[pname])
        ratios, share = temporal_f64.within_bound(got, r, hit, what)
        got2 = gpu_step(b, *frame_args(f), f["spp"], in_place=True, length=False, **PARAMS[pname])
        assert got2[2] is None
        ratios2, _ = temporal_f64.within_bound(got2[:2], without_length(r), hit, what + ", in place")
        found = float((got[2][hit] > f["spp"]).mean())
        print(f"{what}: |diff|/bound colour {max(ratios[0], ratios2[0]):.3f} variance {max(ratios[1], ratios2[1]):.3f} "
              f"length {ratios[2]:.3f}; excluded {share:.4f}; history found {found:.3f}")
        first = k == 0 or (reset and k == len(frames) - 1)
        assert found == 0 if first else found > 0.5, (what, found)
    a.close(), b.close()


def test_device_within_the_f64_bound_under_an_orbit(gpu, oracle):
    """threeSpheres at 64x36 through `temporal_cases.orbit_views`: G-buffers from `DeviceScene.gbuffer`, frames of 8 spp in two
    chunks and their `noise_rgb()` from tracked progressive handles, one seed per frame.  The device's step outputs against the f64
    reference fed the same device arrays; the moved steps find history for more than half of the hit pixels, so the comparison is
    of blended values."""
    t, sd, cam, p = three_spheres(8, 4)
    w, h = p.width, p.height
    ds = render.DeviceScene(sd)
    tm = render.Temporal(w, h)
    r = temporal_f64.TemporalF64(w, h)
    for k, view in enumerate(temporal_cases.orbit_views()):
        c = temporal_cases.orbit_camera(oracle, view, w, h)
        if k == 0:
            assert bytes(c) == bytes(cam)  # the first view is the scene's own camera
        frame, var = tracked_frame(ds, c, p, 100 + k)
        g = ds.gbuffer(c, p)
        ds.query_sync()
        out = tm.step(frame, var, g, c, 8, length=True)
        torch.cuda.synchronize()
        got = tuple(x.cpu().numpy() for x in out)
        rgb, v, idx, nrm, pt = (x.cpu().numpy() for x in (frame, var, g.index, g.normal, g.point))
        ref = r.step(rgb, v, idx, nrm, pt, c, 8, bound=True)
        hit = idx >= 0
        ratios, share = temporal_f64.within_bound(got, ref, hit, f"orbit step {k}")
        found = float((got[2][hit] > 8).mean())
        print(f"orbit step {k}: |diff|/bound {ratios[0]:.3f} {ratios[1]:.3f} {ratios[2]:.3f}; excluded {share:.4f}; history found {found:.3f}")
        assert hit.any() and (found > 0.5 if k else found == 0), (k, found)
        assert r.last_static == (k == 1)
    tm.close(), ds.close()
