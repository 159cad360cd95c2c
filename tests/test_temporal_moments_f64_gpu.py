"""Temporal accumulation's moments mode and feedback on the GPU against the f64 statement of their contracts DIRECTLY
(tests/temporal_moments_f64.py) — not through the CPU mirrors the kernels were written beside: every
colour, variance, length and W2 of every step of `render.Temporal(moments=True)` and of `render.Temporal(moments=True,
feedback=True)` lies within the reference's derived bound, with at most 2 % of a step's hit pixels in either exclusion mask, on a
sequence that moves and turns a general camera over two depth layers with unequal spp — at parameter sets that put the temporal and
the spatial estimate into one step and one workgroup tile — and on device G-buffers and one-chunk frames of threeSpheres under a
camera that orbits and dollies, with the level-1 tap of a guided run fed back.  tests/test_temporal_moments_f64_cpu.py runs the
same sequences, images and orbit on the mirrors."""
import ctypes as C

import numpy as np
import pytest
import torch

import temporal_cases
import temporal_moments_f64 as f64
import test_temporal_moments_f64_cpu as cpu
from rayz_amd import capi, render, tracer
from test_temporal_feedback_gpu import gpu_feedback
from test_temporal_moments_gpu import gpu_step

pytestmark = pytest.mark.gpu

PNAMES = ["defaults", "w2max-half", "w2max-half-binding"]


def report(what, ratios, shares, extra=""):
    print(f"{what}: |diff|/bound " + " ".join(f"{n} {x:.3f}" for n, x in zip(f64.NAMES, ratios))
          + f"; excluded {shares[0]:.4f}, variance {shares[1]:.4f}{extra}")


@pytest.mark.parametrize("reset", [False, True], ids=["straight", "reset-before-last"])
@pytest.mark.parametrize("pname", PNAMES)
@pytest.mark.parametrize("w,h", [(45, 23), (97, 41)])
def test_device_within_the_f64_bound_under_a_moving_camera(gpu, w, h, pname, reset):
    """Two device handles — with the optional outputs (length, W2) and without them — through first, static, moved, turned and
    moved again at spp 4, 8, 16, 8, 4; neither size is a multiple of the 32x8 tile.  With w2_max = 0.5 the moved steps have both
    estimates in one step and in one tile (tests/test_temporal_moments_f64_cpu.py asserts that on the reference's selection)."""
    seq = "moving-reset" if reset else "moving"
    frames, (ref, _) = cpu.frames_of(seq, w, h), cpu.reference(seq, w, h, pname, False)
    a, b = render.Temporal(w, h, moments=True), render.Temporal(w, h, moments=True)
    for k, (f, r) in enumerate(zip(frames, ref)):
        if reset and k == len(frames) - 1:
            a.reset(), b.reset()
        hit = f["index"] >= 0
        what = f"moving {w}x{h} {pname} step {k}"
        got = gpu_step(a, *cpu.frame_args(f, k), **cpu.PARAMS[pname])
        ratios, shares = f64.within_bound(got, r, hit, what)
        got2 = gpu_step(b, *cpu.frame_args(f, k), optional=False, **cpu.PARAMS[pname])
        ratios2, _ = f64.within_bound(got2, r, hit, what + ", no optional outputs")
        found = float((got[2][hit] > f["spp"]).mean())
        report(what, [max(x, y) for x, y in zip(ratios, ratios2 + [0, 0])], shares, f"; history found {found:.3f}")
        first = k == 0 or (reset and k == len(frames) - 1)
        assert found == 0 if first else found > 0.5, (what, found)
    a.close(), b.close()


@pytest.mark.parametrize("reset", [False, True], ids=["straight", "reset-before-last"])
@pytest.mark.parametrize("pname", PNAMES)
@pytest.mark.parametrize("w,h", [(45, 23), (97, 41)])
def test_feedback_handle_within_the_f64_bound_under_a_moving_camera(gpu, w, h, pname, reset):
    """The same sequence through a handle that tracks feedback, `Temporal.feedback` behind every step with the seeded images of
    the CPU test (a NaN and a +inf in hit pixels), against `TemporalMomentsF64(feedback=True)` given the same images."""
    seq = "moving-reset" if reset else "moving"
    frames, (ref, _) = cpu.frames_of(seq, w, h), cpu.reference(seq, w, h, pname, True)
    tm = render.Temporal(w, h, moments=True, feedback=True)
    for k, (f, r) in enumerate(zip(frames, ref)):
        if reset and k == len(frames) - 1:
            tm.reset()
        what = f"moving {w}x{h} {pname} feedback step {k}"
        got = gpu_step(tm, *cpu.frame_args(f, k), **cpu.PARAMS[pname])
        ratios, shares = f64.within_bound(got, r, f["index"] >= 0, what)
        report(what, ratios, shares)
        gpu_feedback(tm, cpu.feedback_image(seq, w, h, k))
    tm.close()


def test_device_within_the_f64_bound_under_an_orbit(gpu, oracle):
    """threeSpheres at 64x36 through `temporal_cases.orbit_views`: G-buffers from `DeviceScene.gbuffer`, frames of 4 spp in ONE
    chunk from `DeviceScene.render_into`, one seed per frame — no variance input exists: the case the mode is for.  Moments handles
    at the orbit's two parameter sets (tests/test_temporal_moments_f64_cpu.py: the defaults with w2_max off the values equal frames
    land on) against the reference fed the same device arrays; then feedback handles fed the level-1 tap of
    `Denoiser.run_guided(out, var, g, tap_level=1)`: the tap is read back and given to the reference as the f32 image it is — an
    input to both sides, not something compared.  The moved steps find history for more than half of the hit pixels."""
    t = tracer.threeSpheres(64, seed=3)
    t.samples_per_px, t.max_bounces = 4, 8
    t.set_gpu(render_seed=17, chunk_spp=0, traversal=capi.TRAVERSAL_BVH, tmin=1e-3)
    sd, p = t.scene_desc(), t.params()
    w, h = p.width, p.height
    sched = (C.c_uint32 * 8)()
    assert capi.load().rayz_hip_chunk_schedule(C.byref(p), sched, 8) == 1  # one chunk: K = 1
    ds, dn = render.DeviceScene(sd), render.Denoiser(w, h)
    handles = {}
    for pname, prm in cpu.ORBIT_PARAMS.items():
        handles[pname, False] = (render.Temporal(w, h, moments=True), f64.TemporalMomentsF64(w, h), prm)
        handles[pname, True] = (render.Temporal(w, h, moments=True, feedback=True), f64.TemporalMomentsF64(w, h, feedback=True), prm)
    for k, view in enumerate(temporal_cases.orbit_views()):
        c = temporal_cases.orbit_camera(oracle, view, w, h)
        q = capi.RenderParams.from_buffer_copy(p)
        q.seed = 100 + k
        frame = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ds.render_into(c, q, frame.data_ptr())
        ds.sync()
        g = ds.gbuffer(c, p)
        ds.query_sync()
        rgb, idx, nrm, pt = (x.cpu().numpy() for x in (frame, g.index, g.normal, g.point))
        hit = idx >= 0
        for (pname, fed), (tm, r, prm) in handles.items():
            out = tm.step_moments(frame, g, c, 4, length=True, w2=True, **prm)
            torch.cuda.synchronize()
            got = tuple(x.cpu().numpy() for x in out)
            ref = r.step(rgb, idx, nrm, pt, c, 4, bound=True, **prm)
            what = f"orbit {pname}{' feedback' if fed else ''} step {k}"
            ratios, shares = f64.within_bound(got, ref, hit, what)
            found = float((got[2][hit] > 4).mean())
            report(what, ratios, shares, f"; history found {found:.3f}; spatial {float(r.last_spatial[hit].mean()):.3f}")
            assert hit.any() and (found > 0.5 if k else found == 0), (what, found)
            assert r.last_static == (k == 1)
            if fed:
                _, tap = dn.run_guided(out[0], out[1], g, tap_level=1)
                tm.feedback(tap)
                torch.cuda.synchronize()
                r.feedback(tap.cpu().numpy())
    for tm, _, _ in handles.values():
        tm.close()
    dn.close(), ds.close()
