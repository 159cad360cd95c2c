"""Hand-derived exact answers for temporal accumulation's background mode, shared by its CPU and GPU tests.

The frames are tests/temporal_cases.py's: the exact camera `cam(ox, oy)`, colours col(a) = (a, a/2, 2a), variance V0 = (1/4, 1/8, 1/2),
4 samples per pixel; a background pixel has index -1 and zeros for its normal and point.  For two such cameras the previous one has
r0' = (8, 0, -ox'), r1' = (0, 8, -oy'), r2' = (0, 0, 1), det' = 8 and this one's columns are (1, 0, 0), (0, 1, 0), (ox, oy, 8), so
G = [[1, 0, ox - ox'], [0, 1, oy - oy'], [0, 0, 1]] exactly: gamma = 1, and the background pixel (px, py) lay at (px + ox - ox',
py + oy - oy') — moving px_origin by (+k, 0, 0) makes it take the record k pixels to its RIGHT.  (A hit pixel of the plane z = 0
moves the same way, tests/temporal_cases.py; the sky differs from it when look_from moves.)

Every step carries `mode`, the handle's background mode while it runs ("input" or "accumulate"), and may carry `counts` as
tests/temporal_counts_cases.py's steps do.  A case is a list of steps and `want` for its LAST step, as in tests/temporal_cases.py
(plain: colour, variance, length) and tests/temporal_moments_cases.py (moments: colour, variance, length, W2)."""
from fractions import Fraction as F

import numpy as np

from temporal_cases import V0, Case, Step, cam, col
from temporal_counts_cases import CMStep, CStep
from temporal_moments_cases import MCase, MStep

HALF = tuple(v / 2 for v in V0)
ZERO3 = (0, 0, 0)


def B(step, mode="accumulate", bg=None):
    """The step in `mode`, with the pixels `bg` ((y, x) pairs; None: every pixel) made background."""
    h, w = step.index.shape
    for p in ([(y, x) for y in range(h) for x in range(w)] if bg is None else bg):
        step.background(*p)
    step.mode = mode
    return step


# ---- the plain handle -----------------------------------------------------------------------------------------------------------
def static_two(mode):
    """Static camera, two steps, col(1) then col(3); (0, 1) is background in both.  ACCUMULATE: its own record is a miss, b = 1:
    hN = 4, a0 = 1/2, c = fma(1/2, 3 - 1, 1) = 2 per unit, v = 1/4·s + 1/4·s = s/2, N = 8 — the hit pixel's static-two.  INPUT: out = in =
    col(3), V0, N = 4.  The hit pixel (0, 0) blends in both modes."""
    steps = [B(Step(3, 2, cam(), 1), mode, [(0, 1)]), B(Step(3, 2, cam(), 3), mode, [(0, 1)])]
    bg = (col(2), HALF, 8) if mode == "accumulate" else (col(3), V0, 4)
    return Case(f"bg-static-two-{mode}", static_two.__doc__, steps, {(0, 1): bg, (0, 0): (col(2), HALF, 8)})


def pan(kx, ky):
    """Every pixel is background.  History base (1 + x + 8y)/16 through cam(0, 0), then colour 0 through cam(kx, ky): G's translation is
    (kx, ky), x = px + kx, fx = 0: the tap (px + kx, py + ky) has b = 1, the other three b = 0.  out = h/2, v = V0/2, N = 8 where that
    pixel exists; where px + kx >= width (not < width) or px + kx <= -1 (not > -1), likewise in y, the projection fails: out = 0, V0, 4."""
    w, h = 5, 4
    base = lambda y, x: F(1 + x + 8 * y, 16)  # noqa: E731
    steps = [B(Step(w, h, cam(0, 0), base)), B(Step(w, h, cam(kx, ky), 0))]
    want = {}
    for y in range(h):
        for x in range(w):
            if 0 <= x + kx < w and 0 <= y + ky < h:
                want[(y, x)] = (tuple(c / 2 for c in col(base(y + ky, x + kx))), HALF, 8)
            else:
                want[(y, x)] = (col(0), V0, 4)
    return Case(f"bg-pan-{kx}-{ky}", pan.__doc__, steps, want)


def half_shift_one_hit():
    """cam(1/2, 0) after cam(0, 0): x = px + 1/2, taps (px, py) and (px + 1, py) with b = 1/2 each.  The history pixel (0, 1) was a HIT
    (index 7), the others misses.  Pixel (0, 0): tap (0, 0) accepted, tap (0, 1) refused by its index: B = 1/2, h = (1/2·c)/(1/2) = c =
    col(1) exactly, current colour 0: out = col(1/2), v = V0/2, N = 8.  Pixel (0, 1): tap (0, 1) refused, tap (0, 2) (base 3) accepted:
    col(3/2).  Pixel (0, 2): taps (0, 2) and (0, 3), bases 3 and 5: h = col(4), out = col(2)."""
    a = B(Step(4, 1, cam(0, 0), lambda y, x: {0: 1, 1: 2, 2: 3, 3: 5}[x]), bg=[(0, 0), (0, 2), (0, 3)])
    b = B(Step(4, 1, cam(F(1, 2), 0), 0))
    want = {(0, 0): (col(F(1, 2)), HALF, 8), (0, 1): (col(F(3, 2)), HALF, 8), (0, 2): (col(2), HALF, 8)}
    return Case("bg-half-shift-one-hit", half_shift_one_hit.__doc__, [a, b], want)


def all_taps_hits():
    """The same move over a history of hits only: no tap of a background pixel is accepted, B = 0: out = in = col(1/2), V0, N = 4."""
    a = B(Step(4, 1, cam(0, 0), 1), bg=[])
    b = B(Step(4, 1, cam(F(1, 2), 0), F(1, 2)))
    return Case("bg-all-taps-hits", all_taps_hits.__doc__, [a, b], {(0, 0): (col(F(1, 2)), V0, 4), (0, 2): (col(F(1, 2)), V0, 4)})


def own_record_was_a_hit():
    """Static, two steps; (0, 1) is background in the SECOND frame only: its own record has index 7, not < 0: out = in = col(3), V0,
    N = 4.  (1, 1) is background in the FIRST frame only: a hit pixel whose record is a miss has no history either, as in INPUT mode."""
    a = B(Step(3, 2, cam(), 1), bg=[(1, 1)])
    b = B(Step(3, 2, cam(), 3), bg=[(0, 1)])
    return Case("bg-own-record-was-a-hit", own_record_was_a_hit.__doc__, [a, b], {(0, 1): (col(3), V0, 4), (1, 1): (col(3), V0, 4)})


def no_parallax():
    """look_from AND px_origin move by (1, 0, 0): a = px_origin - look_from is (0, 0, 8) in both frames, G is the identity — but the
    camera's bytes differ, so the step is NOT static.  Row 0 is background: x = px, fx = 0, its own record with b = 1: out = h/2 with
    h = col(base(0, px)).  Row 1 is the plane z = 0 and sees parallax: its pixel (1, px) reports P = (px + 1, 1, 0), which the previous
    camera cam(0, 0) saw at x = px + 1: it takes the record to its right, and at px = 3 x = 4 is not < 4: no history."""
    w, h = 4, 2
    base = lambda y, x: F(1 + x + 8 * y, 16)  # noqa: E731
    moved = dict(look_from=(1.0, 0.0, -8.0), px_du=(1.0, 0.0, 0.0), px_dv=(0.0, 1.0, 0.0), px_origin=(1.0, 0.0, 0.0))
    row0 = [(0, x) for x in range(w)]
    steps = [B(Step(w, h, cam(0, 0), base), bg=row0), B(Step(w, h, moved, 0), bg=row0)]
    want = {(0, x): (tuple(c / 2 for c in col(base(0, x))), HALF, 8) for x in range(w)}
    want.update({(1, x): (tuple(c / 2 for c in col(base(1, x + 1))), HALF, 8) for x in range(w - 1)})
    want[(1, 3)] = (col(0), V0, 4)
    return Case("bg-no-parallax", no_parallax.__doc__, steps, want)


def weight_threshold():
    """cam(-127/128, 0) after cam(0, 0): x = px - 127/128, x0 = px - 1, fx = 1/128: the taps (px - 1) with b = 127/128 and (px) with b = 1/128.
    History bases 1, 2, 4, 8; the history pixel (0, 1) was a hit.  Pixel 0: the tap at -1 is outside, the tap 0 has b = 1/128 < 2^-6: no
    history, out = in = 0.  Pixel 1: tap 0 accepted (B = 127/128), tap 1 refused: h = (127/128·c)/(127/128) = c = col(1): out = col(1/2).
    Pixel 2: tap 1 refused, tap 2 has b = 1/128: no history.  Pixel 3: taps 2 and 3, B = 127/128 + 1/128 = 1, h = (127·4 + 8)/128 =
    129/32 per unit, exact: out = col(129/64).  The variances are V0 in every record: v = V0/2; N = 8."""
    a = B(Step(4, 1, cam(0, 0), lambda y, x: 2 ** x), bg=[(0, 0), (0, 2), (0, 3)])
    b = B(Step(4, 1, cam(F(-127, 128), 0), 0))
    want = {(0, 0): (col(0), V0, 4), (0, 1): (col(F(1, 2)), HALF, 8), (0, 2): (col(0), V0, 4), (0, 3): (col(F(129, 64)), HALF, 8)}
    return Case("bg-weight-threshold", weight_threshold.__doc__, [a, b], want)


def turned_away():
    """The second camera has px_du = (1, 0, -8), px_dv = (0, 1, 0), a = (0, 0, 8) (det = 8); the first is cam(0, 0): G's rows are
    r0'·c/8 = (1, 0, 0), (0, 1, 0) and r2'·c/8 = (-1, 0, 1): gamma = 1 - px.  Pixel 0: gamma = 1, x = 0, y = 0: its own record, out = h/2.
    Pixel 1: gamma = 0, pixel 2: gamma = -1, neither > 0: the projection fails, out = in = col(1/2), V0, N = 4."""
    turned = dict(look_from=(0.0, 0.0, -8.0), px_du=(1.0, 0.0, -8.0), px_dv=(0.0, 1.0, 0.0), px_origin=(0.0, 0.0, 0.0))
    steps = [B(Step(3, 1, cam(0, 0), 3)), B(Step(3, 1, turned, F(1, 2)))]
    want = {(0, 0): (col(F(7, 4)), HALF, 8), (0, 1): (col(F(1, 2)), V0, 4), (0, 2): (col(F(1, 2)), V0, 4)}
    return Case("bg-turned-away", turned_away.__doc__, steps, want)


def input_then_accumulate():
    """Static, three steps col(1), col(3), col(5); the first two in INPUT mode, the third in ACCUMULATE.  The background pixel (0, 1)
    passed col(3) through in step 2 and left the record {col(3), V0, N = 4, index -1}; step 3 reads it: c = fma(1/2, 5 - 3, 3) = 4, V0/2,
    N = 8.  The mode is no state of the history."""
    steps = [B(Step(3, 2, cam(), 1), "input", [(0, 1)]), B(Step(3, 2, cam(), 3), "input", [(0, 1)]), B(Step(3, 2, cam(), 5), "accumulate", [(0, 1)])]
    return Case("bg-input-then-accumulate", input_then_accumulate.__doc__, steps, {(0, 1): (col(4), HALF, 8)})


def accumulate_then_input():
    """.. and the other way round: two ACCUMULATE steps, then an INPUT step: out = in = col(5), V0, N = 4 at the background pixel."""
    steps = [B(Step(3, 2, cam(), 1), "accumulate", [(0, 1)]), B(Step(3, 2, cam(), 3), "accumulate", [(0, 1)]), B(Step(3, 2, cam(), 5), "input", [(0, 1)])]
    return Case("bg-accumulate-then-input", accumulate_then_input.__doc__, steps, {(0, 1): (col(5), V0, 4)})


# ---- counts -----------------------------------------------------------------------------------------------------------------------
def counts_zero_keeps():
    """Static, counts.  Step 1: col(1), 4 samples.  Step 2, alpha_min = 0.4: the background pixel (0, 0) has count 0 and NaN colour and
    variance; it finds its own record (a miss, N = 4 > 0) and keeps it by selection: col(1), V0, N = 4 — no NaN, alpha_min not applied."""
    steps = [B(CStep(3, 2, cam(), 1), bg=[(0, 0)]), B(CStep(3, 2, cam(), 3, counts={(0, 0): 0}, blank=[(0, 0)], alpha_min=0.4), bg=[(0, 0)])]
    return Case("bg-counts-zero-keeps", counts_zero_keeps.__doc__, steps, {(0, 0): (col(1), V0, 4)})


def counts_length_zero_refused():
    """Static, counts.  Step 1: the background pixel (0, 0) has count 0 on a fresh handle: its record has N = 0 (and a NaN colour).
    Step 2: 4 samples, col(3): its own record is a miss but holds no samples: refused, no history: out = in = col(3), V0, N = 4."""
    steps = [B(CStep(3, 2, cam(), 1, counts={(0, 0): 0}, blank=[(0, 0)]), bg=[(0, 0)]), B(CStep(3, 2, cam(), 3), bg=[(0, 0)])]
    return Case("bg-counts-length-zero-refused", counts_length_zero_refused.__doc__, steps, {(0, 0): (col(3), V0, 4)})


def counts_n_max_binds():
    """Static, counts.  Step 1: 8 samples, col(1).  Step 2 with n_max = 6 and count 0 at the background pixel (0, 0): it keeps col(1) and
    V0, and N = min(8 + 0, 6) = 6."""
    steps = [B(CStep(3, 2, cam(), 1, counts=8), bg=[(0, 0)]), B(CStep(3, 2, cam(), 3, counts={(0, 0): 0}, blank=[(0, 0)], n_max=6.0), bg=[(0, 0)])]
    return Case("bg-counts-n-max-binds", counts_n_max_binds.__doc__, steps, {(0, 0): (col(1), V0, 6)})


def cases():
    out = [static_two("accumulate"), static_two("input")]
    out += [pan(kx, ky) for kx, ky in ((1, 0), (0, 1), (2, 1), (-1, 0), (-2, -1))]
    out += [half_shift_one_hit(), all_taps_hits(), own_record_was_a_hit(), no_parallax(), weight_threshold(), turned_away(),
            input_then_accumulate(), accumulate_then_input(), counts_zero_keeps(), counts_length_zero_refused(), counts_n_max_binds()]
    return out


# ---- the moments handle -----------------------------------------------------------------------------------------------------------
def moments_static_two(w2_max):
    """Static, two moments steps, col(1) then col(3), (0, 1) background in both, ACCUMULATE.  Red: c = 2, m2 = fma(1/2, 9 - 1, 1) = 5,
    W2 = fma(1/4, 1, 1/4) = 1/2, N = 8.  w2_max = 1/2: W2 > 1/2 is false, so v = vt: e = 5 - 4 = 1 = (c1 - c2)²/4, (e·W2)/(1 - W2) = 1;
    green (1/2, 3/2): 1/4; blue (2, 6): 4.  The default w2_max = 1/4: W2 > 1/4, and a background pixel takes no spatial estimate: +0."""
    steps = [B(MStep(3, 2, cam(), 1, w2_max=w2_max), bg=[(0, 1)]), B(MStep(3, 2, cam(), 3, w2_max=w2_max), bg=[(0, 1)])]
    v = (1, F(1, 4), 4) if w2_max == 0.5 else ZERO3
    return MCase(f"bg-moments-static-two-w2max-{w2_max}", moments_static_two.__doc__, steps, {(0, 1): (col(2), v, 8, F(1, 2))})


def moments_input():
    """The same in INPUT mode: out = in = col(3), v = +0, N = 4, W2 = 1."""
    steps = [B(MStep(3, 2, cam(), 1, w2_max=0.5), "input", [(0, 1)]), B(MStep(3, 2, cam(), 3, w2_max=0.5), "input", [(0, 1)])]
    return MCase("bg-moments-input", moments_input.__doc__, steps, {(0, 1): (col(3), ZERO3, 4, 1)})


def moments_counts_zero_keeps():
    """Static, moments counts.  Step 1: col(1), 4 samples: the record {col(1), m2 = col(1)², W2 = 1, N = 4}.  Step 2: count 0 and a NaN
    colour at the background pixel (0, 0): colour, m2, W2 and N are kept by selection; W2 = 1 > w2_max: v = +0."""
    steps = [B(CMStep(3, 2, cam(), 1), bg=[(0, 0)]), B(CMStep(3, 2, cam(), 3, counts={(0, 0): 0}, blank=[(0, 0)]), bg=[(0, 0)])]
    return MCase("bg-moments-counts-zero-keeps", moments_counts_zero_keeps.__doc__, steps, {(0, 0): (col(1), ZERO3, 4, 1)})


def moments_cases():
    return [moments_static_two(0.5), moments_static_two(0.25), moments_input(), moments_counts_zero_keeps()]


def counts_of(step):
    """What a step adds per pixel: its counts array, or its one spp."""
    return step.counts if hasattr(step, "counts") else step.spp
