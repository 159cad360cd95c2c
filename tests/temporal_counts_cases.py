"""Hand-derived exact answers for temporal accumulation's counts step, shared by its CPU and GPU tests.

The frames are tests/temporal_cases.py's: the plane z = 0 through the exact camera `cam(ox, oy)`, every hit with index 7 and the
normal (0, 0, 1), colours col(a) = (a, a/2, 2a), variance V0 = (1/4, 1/8, 1/2).  A step carries `counts`, one sample count per
pixel (an int: that count everywhere; a dict {(y, x): n} over a default), and `blank`, pixels whose input colour and variance are
NaN — what a sparse render leaves where it traced nothing.

A case is a list of steps and, for its LAST step, `want` as in tests/temporal_cases.py (plain: colour, variance, length) and
tests/temporal_moments_cases.py (moments: colour, variance, length, W2): rationals that ARE f32 values, written out in each case
from §4.23's rules."""
from fractions import Fraction as F

import numpy as np

from temporal_cases import V0, Case, Step, cam, col, r32
from temporal_moments_cases import CAP3, MCase, MStep, spatial3

NAN = float("nan")


def _with_counts(step, counts, default, blank):
    h, w = step.index.shape
    step.counts = np.full((h, w), default if isinstance(counts, dict) else counts, np.int32)
    if isinstance(counts, dict):
        for p, n in counts.items():
            step.counts[p] = n
    for p in blank:
        step.rgb[p] = NAN
        if hasattr(step, "var"):
            step.var[p] = NAN
    return step


def CStep(w, h, camera, base, counts=4, default=4, blank=(), **params):
    """A plain step (temporal_cases.Step) with per-pixel counts."""
    return _with_counts(Step(w, h, camera, base, **params), counts, default, blank)


def CMStep(w, h, camera, base, counts=4, default=4, blank=(), **params):
    """A moments step (temporal_moments_cases.MStep) with per-pixel counts."""
    return _with_counts(MStep(w, h, camera, base, **params), counts, default, blank)


HALF = tuple(v / 2 for v in V0)


# ---- the plain handle -----------------------------------------------------------------------------------------------------------
def first_frame_mixed():
    """One step on a fresh handle, counts 0, 4, 12 and 1 among its pixels: no history, so out = in and the variance is V0 whatever
    the count, and N = n — 0 at (0, 0), where the input passes through all the same."""
    s = CStep(3, 2, cam(), lambda y, x: F(1 + x + 4 * y, 8), counts={(0, 0): 0, (0, 1): 4, (0, 2): 12, (1, 0): 1})
    want = {(0, 0): (col(F(1, 8)), V0, 0), (0, 1): (col(F(2, 8)), V0, 4), (0, 2): (col(F(3, 8)), V0, 12), (1, 0): (col(F(5, 8)), V0, 1)}
    return Case("first-frame-mixed-counts", first_frame_mixed.__doc__, [s], want)


def static_zero(then_sampled):
    """Static camera.  Step 1: col(1), 4 samples everywhere.  Step 2 with alpha_min = 0.4: the pixel (0, 0) has count 0 and a NaN
    colour and variance; it finds its own record (N = 4 > 0), so al = 0 BY SELECTION — alpha_min, which would give 0.4, is not
    applied — and c_out = h = col(1), v_out = hv = V0, N_out = hN = 4: the history's bits, no NaN.  (1, 2) has count 4 and col(3):
    a0 = 1/2 >= 0.4, c = 2, v = V0/2, N = 8 as in static-two.  `then_sampled`: a third step, col(3) and 4 samples everywhere,
    alpha_min = 0: at (0, 0) the history is still col(1), V0, 4 — the NaN reached no record — so it blends as static-two: col(2),
    V0/2, 8."""
    steps = [CStep(3, 2, cam(), 1), CStep(3, 2, cam(), 3, counts={(0, 0): 0}, blank=[(0, 0)], alpha_min=0.4)]
    if then_sampled:
        steps.append(CStep(3, 2, cam(), 3))
        return Case("static-zero-then-sampled", static_zero.__doc__, steps, {(0, 0): (col(2), HALF, 8)})
    return Case("static-zero-keeps-history", static_zero.__doc__, steps, {(0, 0): (col(1), V0, 4), (1, 2): (col(2), HALF, 8)})


def three_quarters():
    """Static; step 1 col(1) with 4 samples, step 2 col(5) with 12: hN = 4, n = 12, Ns = 16, a0 = al = 3/4, c = fma(3/4, 5 − 1, 1) = 4 per
    unit, k = 1/4, v = 9/16·s + 1/16·s = 5/8·s, N = 16.  At (1, 1) step 2 has 4 samples as step 1: al = 1/2, c = 3."""
    steps = [CStep(3, 2, cam(), 1), CStep(3, 2, cam(), 5, counts={(1, 1): 4}, default=12)]
    want = {(0, 0): (col(4), tuple(v * F(5, 8) for v in V0), 16), (1, 1): (col(3), HALF, 8)}
    return Case("al-three-quarters", three_quarters.__doc__, steps, want)


def left_empty_then_sampled():
    """Static, three steps; the pixel (0, 0) has count 0 in the first two.  Step 1: no history, its input col(1) passes through and
    its record gets N = 0.  Step 2: its own record has N = 0 and is REFUSED, so again no history: the input col(2) passes, N = 0.
    Step 3 brings 4 samples of col(5): the record is refused once more, c_out = col(5), v_out = V0, N = n = 4 — nothing of col(1) or
    col(2), which were never samples.  (0, 1) has 4 samples every time: the running mean of 1, 2, 5 as static-three computes it."""
    from temporal_cases import blend

    z = {(0, 0): 0}
    steps = [CStep(2, 1, cam(), 1, counts=z), CStep(2, 1, cam(), 2, counts=z), CStep(2, 1, cam(), 5)]
    two = blend(col(2), V0, col(1), V0, 4, 4)
    assert two == (col(F(3, 2)), HALF, 8)
    return Case("left-empty-then-sampled", left_empty_then_sampled.__doc__, steps,
                {(0, 0): (col(5), V0, 4), (0, 1): blend(col(5), V0, two[0], two[1], two[2], 4)})


def half_shift_one_empty_tap():
    """px_origin moves by (−1/2, 0): the pixel (0, px) has the taps (0, px − 1) and (0, px) with b = 1/2 each (the j = 1 row lies outside
    a one-row frame).  History base (1 + x)/8 with 4 samples, except (0, 1), which had count 0: its record (N = 0) is refused like
    a different surface.  Current colour 0, 4 samples.  (0, 2): the tap (0, 1) is refused, B = 1/2, H = base(2)/2, h = base(2) =
    3/8 exactly, hN = (1/2·4)/(1/2) = 4; out = h/2, v = V0/2, N = 8.  (0, 1): the tap (0, 0) alone: h = 1/8.  (0, 3): both taps,
    B = 1, h = (3/8 + 4/8)/2 = 7/16."""
    a = CStep(4, 1, cam(0, 0), lambda y, x: F(1 + x, 8), counts={(0, 1): 0})
    b = CStep(4, 1, cam(F(-1, 2), 0), 0)
    want = {(0, 2): (col(F(3, 16)), HALF, 8), (0, 1): (col(F(1, 16)), HALF, 8), (0, 3): (col(F(7, 32)), HALF, 8)}
    return Case("half-shift-one-empty-tap", half_shift_one_empty_tap.__doc__, [a, b], want)


def all_taps_empty():
    """The same move over a history in which EVERY record has N = 0 (a first frame of counts 0): no tap is accepted, B = 0 is not
    >= 2^-6: no history, out = in = col(1/2), v = V0, N = n = 4."""
    a = CStep(4, 1, cam(0, 0), 1, counts=0)
    b = CStep(4, 1, cam(F(-1, 2), 0), F(1, 2))
    return Case("all-taps-empty", all_taps_empty.__doc__, [a, b], {(0, 2): (col(F(1, 2)), V0, 4), (0, 0): (col(F(1, 2)), V0, 4)})


def n_max_binds_without_samples():
    """Static, n_max = 6.  Step 1: 8 samples of col(1) and no history: N = n = 8 (a first frame's length is its count).  Step 2: count 0
    and a NaN input: c_out = h = col(1), v_out = V0, and N_out = hN > nm ? nm : hN = 6: the cap applies to a pixel that got nothing."""
    steps = [CStep(2, 1, cam(), 1, counts=8, n_max=6.0), CStep(2, 1, cam(), 3, counts=0, blank=[(0, 0), (0, 1)], n_max=6.0)]
    return Case("n-max-binds-without-samples", n_max_binds_without_samples.__doc__, steps, {(0, 0): (col(1), V0, 6), (0, 1): (col(1), V0, 6)})


def cases():
    return [first_frame_mixed(), static_zero(False), static_zero(True), three_quarters(), left_empty_then_sampled(),
            half_shift_one_empty_tap(), all_taps_empty(), n_max_binds_without_samples()]


# ---- the moments handle ---------------------------------------------------------------------------------------------------------
def moments_zero_keeps():
    """Static, w2_max = 1/2, alpha_min = 0.  Steps 1 and 2 are temporal_moments_cases' static-two: col(1) then col(3), 4 samples each:
    c = 2, m2 = 5 (red), W2 = 1/2, N = 8.  Steps 3 and 4: count 0 and a NaN colour at (0, 0): c_out = h = 2, m2_out = hq = 5,
    W2_out = hW = 1/2 by selection, N = 8; W2 is not > 1/2: the temporal estimate from the KEPT moments, e = 5 − 4 = 1,
    v = (1·1/2)/(1 − 1/2) = 1 (green 1/4, blue 4).  Step 4 reads what step 3 stored: the same again."""
    blank = dict(counts={(0, 0): 0}, blank=[(0, 0)], w2_max=0.5)
    steps = [CMStep(3, 2, cam(), 1, w2_max=0.5), CMStep(3, 2, cam(), 3, w2_max=0.5), CMStep(3, 2, cam(), 7, **blank),
             CMStep(3, 2, cam(), 9, **blank)]
    return MCase("moments-zero-keeps-m2-and-W2", moments_zero_keeps.__doc__, steps, {(0, 0): (col(2), (1, F(1, 4), 4), 8, F(1, 2))})


def _ramp(y, x):
    return F(x, 8)


def sampled_neighbourhood():
    """A 7x7 first frame of one surface, base x/8, in which the columns x = 0, 2, 4, 6 have count 0 and the colour col(64) — values
    that would move every sum if they were counted.  (3, 3) has 4 samples: W2 = 1 > w2_max, the spatial estimate over the SAMPLED
    positions x = 1, 3, 5 of all seven rows, 21 taps in tap order; c_out = col(3/8), N = 4.  (3, 2) has count 0: no history, so its
    input col(64) passes through with N = 0, W2 = 1, and its estimate runs over the same 21 taps — the centre itself is NOT
    counted."""
    zero = {(y, x): 0 for y in range(7) for x in (0, 2, 4, 6)}
    s = CMStep(7, 7, cam(), lambda y, x: F(64) if x % 2 == 0 else _ramp(y, x), counts=zero)
    taps = [_ramp(y, x) for y in range(7) for x in (1, 3, 5)]
    v = spatial3(taps)
    assert len(taps) == 21 and v != spatial3(taps + [F(64)]) and v[0] < 1
    return MCase("sampled-neighbourhood", sampled_neighbourhood.__doc__, [s], {(3, 3): (col(F(3, 8)), v, 4, 1), (3, 2): (col(64), v, 0, 1)})


def too_few_sampled():
    """A 3x3 first frame, min_taps = 4, of which only (0, 0), (1, 1) and (2, 1) were sampled: at (1, 1) S0 = 3 < 4: 2^32 — nine taps
    would have passed.  With min_taps = 3 the three taps 0, 1/8, 1/8 give mu = r32(1/12) .. the estimate spatial3 computes."""
    base = lambda y, x: F(x, 8)  # noqa: E731
    zero = {(y, x): 0 for y in range(3) for x in range(3) if (y, x) not in ((0, 0), (1, 1), (2, 1))}
    a = CMStep(3, 3, cam(), base, counts=zero)
    b = CMStep(3, 3, cam(), base, counts=zero, min_taps=3.0)
    three = spatial3([F(0), F(1, 8), F(1, 8)], mt=F(3))
    assert three[0] < CAP3[0]
    return [MCase("too-few-sampled", too_few_sampled.__doc__, [a], {(1, 1): (col(F(1, 8)), CAP3, 4, 1)}),
            MCase("three-sampled", too_few_sampled.__doc__, [b], {(1, 1): (col(F(1, 8)), three, 4, 1)})]


def moments_cases():
    return [moments_zero_keeps(), sampled_neighbourhood()] + too_few_sampled()


assert r32(F(1, 3)) != F(1, 3)  # (r32 rounds: the cases above that avoid it are exact on purpose)
