"""The footprint albedo against a float64 statement of DESIGN.md §4.24, without a GPU: the mean of the matching pixels in numpy
float64 (masks and `np.sum`, no fixed order) on the scenes of tests/footprint_scenes.py.

The bound is derived, not measured.  The albedos are non-negative, so every partial sum is a sum of like-signed terms: each of the
n − 1 adds is off by at most u = 2^-24 of a partial sum that is at most the whole sum, the divide by at most u of the quotient, and
f32(n) is exact (n <= 16): first order (n − 1 + 1)·u·mean = n·u·mean, doubled for what first order drops: |out − mean| <= 2·n·u·mean.
Counts and the two selections (`id < 0`, `n == 0`) are integer decisions on identical inputs: exact.

The composed statement needs no new bound: the filtered albedo is an f32 INPUT of §4.20, so tests/upscale_f64.py fed the mirror's
filtered albedo must hold the upscale mirror fed the same within upscale_f64's own bound."""
import numpy as np
import pytest

import footprint_ref
import footprint_scenes
import upscale_f64 as u64
import upscale_ref
from upscale_ref import Guides

U = 2.0 ** -24
CONFIGS = [(w, h, f, curved) for (w, h) in footprint_scenes.SIZES + [(17, 9)] for f in footprint_scenes.FACTORS for curved in (False, True)]


def statement(g_lo, g_hi, f):
    """§4.24 in float64: (mean (h, w, 3), n (h, w)) with the selections applied."""
    h, w = g_lo.index.shape
    idx = np.asarray(g_hi.index).reshape(h, f, w, f).transpose(0, 2, 1, 3).reshape(h, w, f * f)
    alb = np.asarray(g_hi.albedo, np.float64).reshape(h, f, w, f, 3).transpose(0, 2, 1, 3, 4).reshape(h, w, f * f, 3)
    same = idx == np.asarray(g_lo.index)[..., None]
    n = same.sum(axis=-1)
    with np.errstate(all="ignore"):
        mean = np.sum(np.where(same[..., None], alb, 0.0), axis=2) / n[..., None]
    bg = np.asarray(g_lo.index) < 0
    mean = np.where(bg[..., None], 1.0, np.where((n == 0)[..., None], np.asarray(g_lo.albedo, np.float64), mean))
    return mean, n


@pytest.mark.parametrize("w,h,f,curved", CONFIGS)
def test_the_mirror_is_within_the_derived_bound(w, h, f, curved):
    s = footprint_scenes.pair(w, h, f, 1, curved)
    g_lo, g_hi = s["g_lo"], s["g_hi"]
    assert (g_hi.albedo >= 0).all()  # what the bound assumes
    out, count = footprint_ref.footprint_guides(g_lo, g_hi, f)
    mean, n = statement(g_lo, g_hi, f)
    assert np.array_equal(count, n) and n.max() <= 16
    bg, orphan = g_lo.index < 0, (g_lo.index >= 0) & (n == 0)
    assert (out[bg] == 1.0).all()
    assert np.array_equal(out[orphan].view(np.uint32), g_lo.albedo[orphan].view(np.uint32))  # a selection: the bits
    err = np.abs(out.astype(np.float64) - mean)
    bound = 2 * n[..., None] * U * mean
    sel = (bg | orphan)[..., None]
    ratio = np.where(sel, 0.0, np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err == 0, 0.0, np.inf)))
    print(f"footprint mirror vs f64: {w}x{h} f={f} curved={curved}: max err/bound {ratio.max():.4f}; counts {np.bincount(n.ravel()).tolist()}")
    assert ratio.max() <= 1, (w, h, f, curved, float(ratio.max()))


def test_the_scenes_meet_every_rule():
    """Over the sizes above 2 pixels: background pixels, blocks that match partly, blocks that match whole and pixels nothing matches
    all occur at every factor, the checker is finer than a low-resolution pixel (the point sample differs from the mean), and one
    orphan's albedo holds a negative zero."""
    for (w, h) in footprint_scenes.SIZES:
        if w * h <= 2:
            continue
        for f in footprint_scenes.FACTORS:
            s = footprint_scenes.pair(w, h, f, 1)
            _, n = statement(s["g_lo"], s["g_hi"], f)
            idx = s["g_lo"].index
            assert (idx < 0).any() and (idx == footprint_scenes.ORPHAN).any()
            assert ((idx >= 0) & (n == 0)).any() and ((n > 0) & (n < f * f)).any() and (n == f * f).any(), (w, h, f)
            out, _ = footprint_ref.footprint_guides(s["g_lo"], s["g_hi"], f)
            moved = np.abs(out - s["g_lo"].albedo).max(axis=-1) > 0.05
            assert moved.mean() > 0.2, (w, h, f, float(moved.mean()))
            assert (np.signbit(s["g_lo"].albedo) & (s["g_lo"].albedo == 0)).any()


@pytest.mark.parametrize("f", footprint_scenes.FACTORS)
@pytest.mark.parametrize("curved", (False, True))
def test_the_composed_run_is_within_the_upscale_statement(f, curved):
    """§4.20's float64 statement with the mirror's filtered albedo as its g_lo.albedo holds the upscale mirror within its own bound,
    colour, variance and stage map, at 17x9 and 33x9."""
    for (w, h) in ((17, 9), (33, 9)):
        s = footprint_scenes.pair(w, h, f, 1, curved)
        filtered, _ = footprint_ref.footprint_guides(s["g_lo"], s["g_hi"], f)
        g = Guides(s["g_lo"].index, s["g_lo"].normal, s["g_lo"].point, filtered)
        got = upscale_ref.upscale(s["rgb_lo"], g, s["g_hi"], f, var_rgb=s["var_lo"], flags=upscale_ref.ALBEDO)
        out, cb, var, vb, stage, excluded = u64.upscale_f64(s["rgb_lo"], g, s["g_hi"], f, s["var_lo"], flags=u64.ALBEDO, bound=True)
        keep = ~excluded
        assert excluded.mean() <= 0.001, (w, h, f, curved, int(excluded.sum()))
        assert np.array_equal(got[2][keep], stage[keep])
        for a, b, bd, what in ((got[0], out, cb, "colour"), (got[1], var, vb, "variance")):
            err = np.abs(a.astype(np.float64) - b)
            with np.errstate(all="ignore"):
                q = np.where(bd == 0, np.where(err == 0, 0.0, np.inf), err / bd)[keep]
            assert not np.isnan(q).any() and q.max(initial=0.0) <= 1, (w, h, f, curved, what, float(q.max(initial=0.0)))
            print(f"composed vs upscale_f64: {w}x{h} f={f} curved={curved} {what}: max err/bound {q.max(initial=0.0):.4f}")
