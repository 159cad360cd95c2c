"""Temporal accumulation's counts step on the GPU against the f64 statement of its contract DIRECTLY (tests/temporal_counts_f64.py,
DESIGN.md §4.23) — not through the CPU mirror the kernels were written beside: every output of every step of `render.Temporal.step`
and `step_moments` with an int32 counts tensor lies within the reference's derived bound, or equals it bit for bit (NaN included)
where the reference holds the value by selection from the inputs, with at most 2 % of a step's hit pixels excluded — on a sequence
that moves and turns a general camera over two depth layers, under counts drawn per pixel with NaN inputs wherever the count is 0,
and on a lattice's phases traced sparsely into NaN-filled frames of threeSpheres under a camera that orbits and dollies.
tests/test_temporal_counts_f64_cpu.py runs the same sequences on the mirrors and shows that the inputs reach every rule."""
import numpy as np
import pytest
import torch

import temporal_cases
import temporal_counts_f64 as f64
import test_temporal_counts_f64_cpu as cpu
from rayz_amd import render
from test_temporal_counts_gpu import lattice_phase, moments_step, plain_step
from test_temporal_gpu import three_spheres

pytestmark = pytest.mark.gpu


def report(what, ratios, shares, equal, found):
    print(f"{what}: |diff|/bound " + " ".join(f"{n} {x:.3f}" for n, x in zip(f64.NAMES, ratios))
          + f"; excluded {shares[0]:.4f}, variance {shares[1]:.4f}; {equal} values by equality; history found {found:.3f}")


def worst(a, b):
    return [max(x, y) for x, y in zip(a, list(b) + [0.0] * (len(a) - len(b)))]


def run(w, h, moments, pname, reset):
    """Two device handles through a listed sequence — plain: out of place with the length and in place without it; moments: with
    the optional outputs and without them — each step held to the reference's."""
    seq = "moving-reset" if reset else "moving"
    frames, (ref, seen) = cpu.frames_of(seq, w, h), cpu.reference(seq, w, h, moments, pname)
    prm = cpu.params_of(moments)[pname]
    a, b = render.Temporal(w, h, moments=moments), render.Temporal(w, h, moments=moments)
    for k, (f, r, s) in enumerate(zip(frames, ref, seen)):
        first = k == 0 or (reset and k == len(frames) - 1)
        if reset and k == len(frames) - 1:
            a.reset(), b.reset()
        hit = f["index"] >= 0
        what = f"{seq} {w}x{h} {'moments' if moments else 'plain'} {pname} step {k}"
        if moments:
            got, got2 = moments_step(a, f, **prm), moments_step(b, f, optional=False, **prm)
        else:
            got, got2 = plain_step(a, f, **prm), plain_step(b, f, in_place=True, length=False, **prm)
        assert len(got) == (4 if moments else 3) and len(got2) == 2
        ratios, shares, equal = f64.within_bound(got, r, hit, what, s[0])
        ratios2, _, _ = f64.within_bound(got2, r, hit, what + (", no optional outputs" if moments else ", in place"), s[0])
        found = float((got[2][hit] > f["counts"][hit]).mean())  # a length beyond the pixel's own count
        report(what, worst(ratios, ratios2), shares, equal, found)
        assert equal > 0, what
        assert found == 0 if first else found > 0.5, (what, found)
    a.close(), b.close()


@pytest.mark.parametrize("reset", [False, True], ids=["straight", "reset-before-last"])
@pytest.mark.parametrize("pname", ["defaults", "binding"])
@pytest.mark.parametrize("w,h", [(45, 23), (97, 41)])
def test_device_within_the_f64_bound_under_a_moving_camera(gpu, w, h, pname, reset):
    """The plain counts step through first, static, moved, turned and moved again (the static and the moving kernel); neither size is
    a multiple of the 32x8 tile."""
    run(w, h, False, pname, reset)


@pytest.mark.parametrize("reset", [False, True], ids=["straight", "reset-before-last"])
@pytest.mark.parametrize("pname", ["w2max-half", "all-spatial-2-taps"])
@pytest.mark.parametrize("w,h", [(45, 23), (97, 41)])
def test_moments_device_within_the_f64_bound_under_a_moving_camera(gpu, w, h, pname, reset):
    """The moments counts step on the same sequence: with w2_max = 0.5 both estimates meet in one step, and at 97x41 there are tiles
    with and without a spatial pixel; with w2_max = 0 every hit pixel takes the neighbourhood of sampled positions."""
    run(w, h, True, pname, reset)


def test_a_lattice_under_an_orbit_within_the_f64_bound(gpu, oracle):
    """The real pipeline, once: threeSpheres at 64x36, 8 spp in two chunks, through `temporal_cases.orbit_views`.  Each view's frame
    is ONE phase of an f = 2 lattice, traced with `render_pixels` into NaN-filled frames, and is stepped with `render.lattice_counts`
    through a plain handle; the f64 reference is fed the same device arrays.  Every output within the bound or equal by selection,
    under the cap; on the moved steps more than half of the sampled hit pixels find history."""
    t, sd, cam, p = three_spheres(8, 4)
    w, h = p.width, p.height
    ds = render.DeviceScene(sd)
    tm, r = render.Temporal(w, h), f64.TemporalF64(w, h)
    phases = list(render.phase_sequence(2))
    for k, view in enumerate(temporal_cases.orbit_views()):
        c = temporal_cases.orbit_camera(oracle, view, w, h)
        frame, var, counts = lattice_phase(ds, c, p, 100 + k, 2, phases[k % len(phases)], True)
        g = ds.gbuffer(c, p)
        ds.query_sync()
        out = tm.step(frame, var, g, c, counts, length=True)
        torch.cuda.synchronize()
        got = tuple(x.cpu().numpy() for x in out)
        rgb, v, idx, nrm, pt, n = (x.cpu().numpy() for x in (frame, var, g.index, g.normal, g.point, counts))
        n = n.reshape(h, w)
        ref = r.step(rgb, v, idx, nrm, pt, c, n, bound=True)
        f64.no_nan_where_sampled(ref, f"lattice orbit step {k}")
        hit = idx >= 0
        ratios, shares, equal = f64.within_bound(got, ref, hit, f"lattice orbit step {k}", r.last_passthrough)
        sampled = hit & (n > 0)
        found = float((got[2][sampled] > n[sampled]).mean())
        report(f"lattice orbit step {k}", ratios, shares, equal, found)
        assert sampled.any() and 0.2 < float((n > 0).mean()) < 0.3 and np.isnan(rgb[n == 0]).all(), k
        assert r.last_static == (k == 1)
        assert found == 0 if k == 0 else (found > 0.5 or k == 1), (k, found)  # (the static step meets a record no frame has sampled yet)
    tm.close(), ds.close()
