"""Temporal accumulation's background mode on the GPU against its f64 statement DIRECTLY, for the six kernels the plain scalar
statement does not reach (tests/temporal_background_f64.py, DESIGN.md §4.27 with §4.23): `render.Temporal(background="accumulate")`
through the moments handle with one spp, the plain handle with an int32 counts tensor, and the moments handle with counts — every
output of every BACKGROUND pixel of every step within the reference's derived bound, or equal to it bit for bit (NaN included) where
the reference holds the value by selection from the inputs, with at most 2 % of a step's background excluded.
tests/test_temporal_background_f64_cpu.py runs the same sequences on the mirror; tests/test_temporal_background_gpu.py holds the
plain scalar step."""
import functools

import numpy as np
import pytest

import temporal_background_f64 as f64
import temporal_counts_f64 as counts_f64
import test_temporal_background_f64_cpu as cpu
from rayz_amd import render
from test_temporal_background_gpu import moments_step, plain_step

pytestmark = pytest.mark.gpu

CASES = [("moments", "defaults"), ("moments", "w2max-0.45"), ("plain-counts", "defaults"), ("plain-counts", "binding"),
         ("moments-counts", "w2max-0.45"), ("moments-counts", "w2max-0.45-binding")]


@functools.lru_cache(maxsize=None)
def reference(w, h, kind, pname, reset):
    """(frames, the f64 reference's per-step results with bounds and masks, its per-step passthrough mask) of moving_sequence,
    with the history forgotten before the last step if `reset`; computed once, never changed."""
    moments = kind != "plain-counts"
    frames = cpu.frames_of("moving", w, h, kind != "moments")
    r = (f64.TemporalBackgroundMomentsF64 if moments else f64.TemporalBackgroundF64)(w, h)
    out, passed = [], []
    for k, f in enumerate(frames):
        if reset and k == len(frames) - 1:
            r.reset()
        out.append(cpu.step(r, f, moments, bound=True, **cpu.params_of(kind)[pname]))
        passed.append(r.last_passthrough.copy())
    return frames, out, passed


@pytest.mark.parametrize("reset", [False, True], ids=["straight", "reset-before-last"])
@pytest.mark.parametrize("kind,pname", CASES, ids=[f"{k}-{p}" for k, p in CASES])
@pytest.mark.parametrize("w,h", [(45, 23), (97, 41)])
def test_device_within_the_f64_bound_under_a_moving_camera(gpu, w, h, kind, pname, reset):
    """First, static, moved, turned and moved again in ACCUMULATE mode: the static and the moving kernel of `temporal_bg_moments`,
    `temporal_bg_counts` and `temporal_bg_counts_moments`; neither size is a multiple of the 32x8 tile.  Behind a first step more
    than half of the sampled background finds history (three in ten with counts, where two records in five hold no samples)."""
    moments = kind != "plain-counts"
    frames, ref, passed = reference(w, h, kind, pname, reset)
    prm = cpu.params_of(kind)[pname]
    tm = render.Temporal(w, h, moments=moments, background="accumulate")
    for k, (f, r, s) in enumerate(zip(frames, ref, passed)):
        first = k == 0 or (reset and k == len(frames) - 1)
        if reset and k == len(frames) - 1:
            tm.reset()
        bg = f["index"] < 0
        what = f"moving {w}x{h} {kind} {pname} step {k}"
        got = (moments_step if moments else plain_step)(tm, f, **prm)
        ratios, shares, equal = counts_f64.within_bound(got, r, bg, what, s, region=bg)
        n = np.broadcast_to(f["spp"], bg.shape)
        sampled = bg & (n > 0)
        found = float((got[2][sampled] > n[sampled]).mean())
        print(f"{what}: |diff|/bound " + " ".join(f"{x:.3f}" for x in ratios) + f"; excluded {shares[0]:.4f}, variance {shares[1]:.4f}; "
              f"{equal} values by equality; history found {found:.3f}")
        assert found == 0 if first else found > (0.5 if kind == "moments" else 0.3), (what, found)
    tm.close()
