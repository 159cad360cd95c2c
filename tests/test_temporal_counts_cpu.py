"""Temporal accumulation's counts step on the CPU: the restatement tests/temporal_counts_mirror.cpp meets the
hand-derived answers of tests/temporal_counts_cases.py bit for bit; with uniform counts it IS the scalar steps' mirrors
(tests/temporal_mirror.cpp, tests/temporal_moments_mirror.cpp) bit for bit, outputs and history, on the plane, general and moving
sequences — equivalence (a); under a still camera a pixel with count 0 keeps its record — equivalence (b); and
`render.lattice_counts` marks exactly `render.lattice_pixels`' pixels."""
import numpy as np
import pytest

import temporal_cases
import temporal_counts_cases
import temporal_counts_ref
import temporal_moments_ref
import temporal_ref
from rayz_amd import render

ORIGINS = [(0, 0), (0, 0), (0.25, -0.625), (1.25, 0.375)]
BINDING = dict(alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ; first at {bad[:5].tolist()}"


def sequences():
    return [("plane", temporal_cases.plane_sequence(33, 9, 3309, ORIGINS)), ("general", temporal_cases.general_sequence(45, 23, 248)),
            ("moving", temporal_cases.moving_sequence(45, 23, 71))]


@pytest.mark.parametrize("case", temporal_counts_cases.cases(), ids=lambda c: c.name)
def test_mirror_gives_the_hand_derived_answers(case):
    h, w = case.steps[0].index.shape
    rgb, var, length = case.run(temporal_counts_ref.TemporalCounts(w, h),
                                lambda tm, s: tm.step(s.rgb, s.var, s.index, s.normal, s.point, s.camera, s.counts, **s.params))
    case.check(rgb, var, length, "mirror")


@pytest.mark.parametrize("case", temporal_counts_cases.moments_cases(), ids=lambda c: c.name)
def test_moments_mirror_gives_the_hand_derived_answers(case):
    h, w = case.steps[0].index.shape
    out = case.run(temporal_counts_ref.TemporalMomentsCounts(w, h),
                   lambda tm, s: tm.step(s.rgb, s.index, s.normal, s.point, s.camera, s.counts, **s.params))
    case.check(*out, "mirror")
    assert all((a == a).all() for a in out[1:])


@pytest.mark.parametrize("prm", [{}, BINDING], ids=["defaults", "binding"])
def test_uniform_counts_are_the_scalar_step(prm):
    """Equivalence (a), plain: every output and every record of the history, bit for bit, `moving_sequence`'s unequal spp included."""
    for name, frames in sequences():
        h, w = frames[0]["index"].shape
        a, b = temporal_ref.Temporal(w, h), temporal_counts_ref.TemporalCounts(w, h)
        for k, f in enumerate(frames):
            spp = f.get("spp", 8)
            args = (f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"])
            want, got = a.step(*args, spp, **prm), b.step(*args, np.full((h, w), spp), **prm)
            for x, y, what in zip(got, want, ("colour", "variance", "length")):
                same_bits(x, y, f"{name} step {k} {what}")
            for x, y in zip(b.state(), a.state()):
                same_bits(x, y, f"{name} step {k} history")
        assert a.last_static == b.last_static


@pytest.mark.parametrize("prm", [{}, dict(BINDING, w2_max=0.0, min_taps=49.0), dict(w2_max=1.0, min_taps=2.0)], ids=["defaults", "binding", "ends"])
def test_uniform_counts_are_the_scalar_moments_step(prm):
    """Equivalence (a), moments."""
    for name, frames in sequences():
        h, w = frames[0]["index"].shape
        a, b = temporal_moments_ref.TemporalMoments(w, h), temporal_counts_ref.TemporalMomentsCounts(w, h)
        for k, f in enumerate(frames):
            spp = f.get("spp", 8)
            args = (f["rgb"], f["index"], f["normal"], f["point"], f["camera"])
            want, got = a.step(*args, spp, **prm), b.step(*args, spp, **prm)
            for x, y, what in zip(got, want, ("colour", "variance", "length", "W2")):
                same_bits(x, y, f"{name} step {k} {what}")
            for x, y in zip(b.state(), a.state()):
                same_bits(x, y, f"{name} step {k} history")


def test_a_still_camera_keeps_unsampled_records():
    """Equivalence (b): two sampled static frames, then frames in which a random half of the pixels has count 0 and NaN inputs: those
    pixels' records — colour, variance, moments, length — are what they were, bit for bit, step after step; nothing is NaN."""
    w, h = 33, 9
    frames = temporal_cases.plane_sequence(w, h, 12, [(0, 0)] * 5)
    plain, mom = temporal_counts_ref.TemporalCounts(w, h), temporal_counts_ref.TemporalMomentsCounts(w, h)
    rng = np.random.default_rng(5)
    for k, f in enumerate(frames):
        counts = np.full((h, w), 8) if k < 2 else np.where(rng.random((h, w)) < 0.5, 0, 8)
        rgb, var = f["rgb"].copy(), f["var"].copy()
        rgb[counts == 0] = np.nan
        var[counts == 0] = np.nan
        before_p, before_m = plain.state(), mom.state()
        out = plain.step(rgb, var, f["index"], f["normal"], f["point"], f["camera"], counts)
        mout = mom.step(rgb, f["index"], f["normal"], f["point"], f["camera"], counts)
        if k < 2:
            continue
        kept = (counts == 0) & (f["index"] >= 0)
        assert kept.sum() > 50 and plain.last_static and mom.last_static
        for x, y in zip(plain.state()[:2], before_p[:2]):
            same_bits(x[kept], y[kept], f"step {k} plain record")
        for x, y in zip((mom.state()[0], mom.state()[4]), (before_m[0], before_m[4])):
            same_bits(x[kept], y[kept], f"step {k} moments record")
        same_bits(out[0][kept], before_p[0][..., :3][kept], "colour output")
        same_bits(out[2][kept], before_p[0][..., 3][kept], "length output")
        hit = f["index"] >= 0
        assert all(np.isfinite(a[hit]).all() for a in out + mout)


def test_lattice_counts_marks_the_lattice():
    for f in (2, 3, 4):
        w, h = 12 * 2, 12
        total = np.zeros((h, w), np.int64)
        for phase in render.phase_sequence(f):
            c = render.lattice_counts(w, h, f, phase, 7).numpy()
            pixels, _ = render.lattice_pixels(w, h, f, phase)
            want = np.zeros(h * w, np.int32)
            want[pixels.numpy()] = 7
            assert c.dtype == np.int32 and np.array_equal(c.reshape(-1), want)
            total += c
        assert (total == 7).all()  # the phases of one cycle sample every pixel once
    with pytest.raises(ValueError):
        render.lattice_counts(10, 10, 4, (0, 0), 1)
    with pytest.raises(ValueError):
        render.lattice_counts(8, 8, 2, (2, 0), 1)
    with pytest.raises(ValueError):
        render.lattice_counts(8, 8, 2, (0, 0), -1)
