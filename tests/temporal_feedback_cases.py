"""Hand-derived exact answers for temporal accumulation's feedback mode, shared by its CPU and GPU tests.

The frames are tests/temporal_cases.py's: the plane z = 0 through the exact camera `cam(ox, oy)`, every hit with index 7 and the
normal (0, 0, 1); colours are grey(a) = (a, a, a) where a case speaks of one value per pixel, and col(a) = (a, a/2, 2a) where the
channels should differ.  4 spp per frame throughout.

A case is a list of operations — ("step", FStep), ("feedback", image) or ("reset",) — and, for its LAST step, `want`:
{(y, x): (colour, variance, length, W2)} as rationals that ARE f32 values, each written out in the case from §4.17's formulas with
`r32` (one correct rounding, decided in rationals) applied where the contract rounds once; every other value is exact (`R`)."""
from fractions import Fraction as F

import numpy as np

from denoise_cases import R
from temporal_cases import NAN, INF, Step, cam, col, r32
from temporal_moments_cases import CAP3, MWIDE, MCase


def grey(a):
    a = F(a)
    return (a, a, a)


class FStep(Step):
    """A frame whose pixel (y, x) has the colour colour(y, x) (a triple of rationals; or one triple for every pixel)."""

    def __init__(self, w, h, camera, colour, spp=4, **params):
        super().__init__(w, h, camera, 0, spp=spp)
        self.params = {**MWIDE, **params}
        for y in range(h):
            for x in range(w):
                self.rgb[y, x] = [float(c) for c in (colour(y, x) if callable(colour) else colour)]


def image(w, h, colour):
    """A feedback image: (h, w, 3) float32 of colour(y, x) (floats allowed: NaN, inf) or of one triple."""
    a = np.empty((h, w, 3), np.float32)
    for y in range(h):
        for x in range(w):
            a[y, x] = [float(c) for c in (colour(y, x) if callable(colour) else colour)]
    return a


class FCase(MCase):
    def __init__(self, name, why, ops, want):
        super().__init__(name, why, [op[1] for op in ops if op[0] == "step"], want)
        self.ops = ops

    def run(self, handle, step_fn, feedback_fn):
        """Feeds the operations to `handle` through step_fn(handle, step) -> (rgb, var, length, w2), feedback_fn(handle, image) and
        handle.reset(); returns the last step's outputs."""
        out = None
        for op in self.ops:
            if op[0] == "step":
                out = step_fn(handle, op[1])
            elif op[0] == "feedback":
                feedback_fn(handle, op[1])
            else:
                handle.reset()
        return out


B_OPS = [("step", FStep(1, 1, cam(), grey(1), alpha_min=0.0, w2_max=1.0)), ("feedback", image(1, 1, grey(F(1, 4)))),
         ("step", FStep(1, 1, cam(), grey(0), alpha_min=0.0, w2_max=1.0))]
B_WANT = {(0, 0): (grey(F(1, 8)), grey(F(1, 4)), 8, F(1, 2))}


def fed_back_once():
    """(B) 1x1, static, alpha_min = 0, w2_max = 1.  Frame 1, c = 1: no history, colour = m1 = 1, m2 = 1, W2 = 1, N = 4.  Feedback 1/4:
    the colour record is 1/4, m1 stays 1.  Frame 2, c = 0: hN = 4, Ns = 8, al = k = 1/2; colour = fma(1/2, 0 − 1/4, 1/4) = 1/8;
    m1' = fma(1/2, 0 − 1, 1) = 1/2; m2' = fma(1/2, 0 − 1, 1) = 1/2; W2' = fma(1/4, 1, 1/4) = 1/2, not > 1: step 3,
    v = max(1/2 − (1/2)², 0)·(1/2) / (1 − 1/2) = 1/4 — the variance of the mean of the raw 1 and 0.  From the returned colour it
    would be 1/2 − 1/64 = 31/64."""
    return FCase("B-fed-back-once", fed_back_once.__doc__, B_OPS, B_WANT)


def third_frame():
    """(C) .. then a third frame, alpha_min = 1/2, c = 1/2, no new feedback: the history colour is the returned 1/8, m1 = 1/2,
    m2 = 1/2, W2 = 1/2, N = 8.  Ns = 12, a0 = r32(4/12) < 1/2: al = k = 1/2.  colour = fma(1/2, 1/2 − 1/8, 1/8) = 5/16;
    m1' = fma(1/2, 1/2 − 1/2, 1/2) = 1/2; m2' = fma(1/2, 1/4 − 1/2, 1/2) = 3/8; W2' = fma(1/4, 1/2, 1/4) = 3/8;
    v = ((3/8 − 1/4)·3/8) / (1 − 3/8) = (3/64) / (5/8), the one rounded operation; N = 12."""
    ops = B_OPS + [("step", FStep(1, 1, cam(), grey(F(1, 2)), alpha_min=0.5, w2_max=1.0))]
    v = r32(R(F(1, 8) * F(3, 8), "e·W2") / F(5, 8))
    assert v != F(3, 40) and abs(v - F(3, 40)) < F(1, 2 ** 26)
    return FCase("C-third-frame", third_frame.__doc__, ops, {(0, 0): (grey(F(5, 16)), grey(v), 12, F(3, 8))})


def _raw(y, x):
    return F(1 + x + 4 * y, 8)


def _fed(y, x):
    return F(3 + 2 * x + y, 16)


def pan_over_a_fed_back_ramp():
    """(D) 5x2, alpha_min = 0, w2_max = 1/2.  Frame 1 through cam(0, 0): col(raw), raw = (1 + x + 4y)/8.  Feedback: col(fed),
    fed = (3 + 2x + y)/16.  Frame 2 through cam(−1, 0), colour 0: the pixel (y, px) lay at (px − 1, y): fx = fy = 0, the tap
    (px − 1, y) has b = 1 and the other three b = 0 (+ 0 to every sum).  al = 1/2: colour = fed(y, px − 1)/2 per unit — the
    NEIGHBOUR's fed-back value —, m1' = raw(y, px − 1)/2 — the neighbour's RAW value —, m2' = raw²/2, W2 = 1/2, not > 1/2:
    v = (raw²/2 − raw²/4)·(1/2)/(1/2) = raw²/4 per channel, all exact; N = 8.  At px = 0 x = −1 fails x > −1: no history, colour 0,
    N = 4, W2 = 1 > 1/2: the spatial estimate over a frame of zeros, 6 taps at (0, 0): 0."""
    ops = [("step", FStep(5, 2, cam(0, 0), lambda y, x: col(_raw(y, x)), alpha_min=0.0, w2_max=0.5)),
           ("feedback", image(5, 2, lambda y, x: col(_fed(y, x)))),
           ("step", FStep(5, 2, cam(-1, 0), col(0), alpha_min=0.0, w2_max=0.5))]
    want = {(0, 0): (col(0), (0, 0, 0), 4, 1)}
    for y in range(2):
        for x in range(1, 5):
            want[(y, x)] = (tuple(c / 2 for c in col(_fed(y, x - 1))), tuple(R(c * c / 4, "v") for c in col(_raw(y, x - 1))), 8, F(1, 2))
    return FCase("D-pan-over-a-fed-back-ramp", pan_over_a_fed_back_ramp.__doc__, ops, want)


def non_finite_feedback():
    """(E) 3x1, static, alpha_min = 0, w2_max = 1/2.  Frame 1 col(1).  The feedback image is (NaN, 1/4, 1/4) at x = 0, col(1/4) at
    x = 1 and (1/4, +inf, 1/4) at x = 2: the pixels 0 and 2 keep col(1) — all three channels, not only the bad one —, the pixel 1
    takes col(1/4).  Frame 2, colour 0, al = 1/2: colours col(1)/2, col(1/4)/2, col(1)/2; m1' = col(1)/2 and m2' = col(1)²/2
    everywhere: v = col(1)²/4 = (1/4, 1/16, 1); W2 = 1/2, N = 8."""
    fb = {0: (NAN, 0.25, 0.25), 1: col(F(1, 4)), 2: (0.25, INF, 0.25)}
    ops = [("step", FStep(3, 1, cam(), col(1), alpha_min=0.0, w2_max=0.5)), ("feedback", image(3, 1, lambda y, x: fb[x])),
           ("step", FStep(3, 1, cam(), col(0), alpha_min=0.0, w2_max=0.5))]
    v = (F(1, 4), F(1, 16), 1)
    want = {(0, 0): (col(F(1, 2)), v, 8, F(1, 2)), (0, 1): (col(F(1, 8)), v, 8, F(1, 2)), (0, 2): (col(F(1, 2)), v, 8, F(1, 2))}
    return FCase("E-non-finite-feedback", non_finite_feedback.__doc__, ops, want)


def second_feedback_wins():
    """(F) (B) with a feedback of 3/4 given first and the 1/4 after it, before the second frame: the second replaces the first, the
    answers are (B)'s."""
    ops = [B_OPS[0], ("feedback", image(1, 1, grey(F(3, 4)))), B_OPS[1], B_OPS[2]]
    return FCase("F-second-feedback-wins", second_feedback_wins.__doc__, ops, B_WANT)


def reset_forgets_the_feedback():
    """(G) Frame 1, feedback 1/4, rayz_hip_temporal_reset, a frame of c = 1/2: a first frame — colour 1/2, N = 4, W2 = 1, which is not
    > w2_max = 1: step 3 gives (0·1) / (1 − 1) = NaN, which clamps to 2^32."""
    ops = [B_OPS[0], B_OPS[1], ("reset",), ("step", FStep(1, 1, cam(), grey(F(1, 2)), alpha_min=0.0, w2_max=1.0))]
    return FCase("G-reset", reset_forgets_the_feedback.__doc__, ops, {(0, 0): (grey(F(1, 2)), CAP3, 4, 1)})


def cases():
    return [fed_back_once(), third_frame(), pan_over_a_fed_back_ramp(), non_finite_feedback(), second_feedback_wins(),
            reset_forgets_the_feedback()]
