"""Hand-derived exact answers for temporal accumulation's clip mode, shared by its CPU and GPU tests.

The frames are tests/temporal_cases.py's: the plane z = 0 through the exact camera `cam(ox, oy)`, every hit with index 7 and the
normal (0, 0, 1), colours col(a) = (a, a/2, 2a), 4 samples per pixel, alpha_min = 0, n_max = inf, normal_cos_min = 1/2.  A hit pixel
(px, py) of a frame through cam(-1, 0) after cam(0, 0) lay at (px - 1, py): it takes the record to its LEFT with b = 1, and column 0
has no history.  A background pixel of a frame through cam(1, 0) after cam(0, 0) takes the record to its RIGHT
(tests/temporal_background_cases.py).  With one frame of history and 4 samples each, hN = 4, Ns = 8, al = k = 1/2: the blend is
(c + hk)/2 and the plain step's variance V0/2, N = 8.

THE BOX FRAME.  Q is 4x4 with the base values 3 3 3 3 / 5 5 5 5 / 2 2 6 6 / 1 1 7 7: four each of 4 ± 1, two each of 4 ± 2 and 4 ± 3.
Every pixel of a 4x4 frame sees all 16 (the 7x7 window covers the frame: a corner pixel's 16 taps), so for every pixel, red:
S0 = 16, S1 = 64, mu = 4, S2 = 16·16 + (4·1 + 4·1 + 2·4 + 2·4 + 2·9 + 2·9) = 256 + 60 = 316, S2/S0 = 79/4, d = 79/4 - 16 = 15/4,
(d·16)/15 = 4, sd = 2 — every value exact.  Green is red/2: mu = 2, S2/S0 = 79/16, d = 15/16, vn = 1, sd = 1.  Blue is 2·red: mu = 8,
S2/S0 = 79, d = 15, vn = 16, sd = 4.  So gamma = 1 gives the boxes [2, 6], [1, 3], [4, 12], gamma = 1/2 gives [3, 5], [3/2, 5/2],
[6, 10], gamma = 0 gives [mu, mu] and gamma = +inf gives e = +inf: no clip.

Every step carries `mode` (the background mode), `clip`, `gamma` and `min_taps` (the handle's clip mode while it runs).  A case is a
list of steps, `want` for its LAST step as in tests/temporal_cases.py (plain: colour, variance, length) and
tests/temporal_moments_cases.py (moments: colour, variance, length, W2), and `clipped`: {(y, x): 0 or 1} of the last step's map."""
from fractions import Fraction as F

from temporal_cases import V0, Case, Step, cam, col, r32
from temporal_moments_cases import MCase, MStep, clamp

INF = float("inf")
HALF = tuple(v / 2 for v in V0)
Q = ((3, 3, 3, 3), (5, 5, 5, 5), (2, 2, 6, 6), (1, 1, 7, 7))
WILD = 100  # a colour that would move every box if its tap were accepted


def q(y, x):
    return Q[y][x] if x < 4 else WILD


def K(step, clip="variance", gamma=1.0, min_taps=4.0, mode="input", bg=()):
    """The step on a handle in `clip` mode with these parameters and background `mode`; the pixels `bg` made background."""
    for p in bg:
        step.background(*p)
    step.clip, step.gamma, step.min_taps, step.mode = clip, gamma, min_taps, mode
    return step


def paint(step, colours):
    """The step with the colours of the pixels {(y, x): (r, g, b)} replaced."""
    for p, c in colours.items():
        step.rgb[p] = [float(v) for v in c]
    return step


def mean(a, b):
    return tuple((F(x) + F(y)) / 2 for x, y in zip(a, b))


class ClipCase(Case):
    def __init__(self, name, why, steps, want, clipped):
        super().__init__(name, why, steps, want)
        self.clipped = clipped


class ClipMCase(MCase):
    def __init__(self, name, why, steps, want, clipped):
        super().__init__(name, why, steps, want)
        self.clipped = clipped


# ---- the plain handle -----------------------------------------------------------------------------------------------------------
def ghost(clip):
    """5x4.  History col(1) through cam(0, 0), then colour 0 everywhere through cam(-1, 0).  The current neighbourhood of every pixel is
    a constant 0: S1 = S2 = 0, mu = 0, d = 0, sd = 0, e = 1·0 = 0: the box is [0, 0], h = 1 > 0 is clipped to hk = 0 in every channel
    and c_out = fma(1/2, 0 - 0, 0) = 0.  OFF: c_out = fma(1/2, 0 - 1, 1) = 1/2 per unit.  The variance V0/2 and N = 8 are the same in
    both — they ignore the clip.  Column 0 has no history: out = in = 0, V0, 4, not clipped."""
    steps = [K(Step(5, 4, cam(0, 0), 1), clip), K(Step(5, 4, cam(-1, 0), 0), clip)]
    c = col(0) if clip == "variance" else col(F(1, 2))
    want = {(1, 2): (c, HALF, 8), (3, 4): (c, HALF, 8), (1, 0): (col(0), V0, 4)}
    flag = 1 if clip == "variance" else 0
    return ClipCase(f"clip-ghost-{clip}", ghost.__doc__, steps, want, {(1, 2): flag, (3, 4): flag, (1, 0): 0})


HISTORY = {(0, 0): col(4), (1, 0): (7, 2, 8), (2, 0): col(1), (3, 0): col(6), (1, 2): (5, F(7, 2), 2)}


def box(gamma, min_taps=4.0, name=None):
    """4x4.  History: col(4) everywhere but (1, 0) = (7, 2, 8), (2, 0) = col(1) = (1, 1/2, 2), (3, 0) = col(6) = (6, 3, 12) and (1, 2) =
    (5, 7/2, 2), through cam(0, 0); then the box frame Q through cam(-1, 0): pixel (y, x) takes the history of (y, x - 1).  gamma = 1,
    boxes [2, 6], [1, 3], [4, 12]:
      (0, 1): h = (4, 2, 8) inside, untouched: c = col(3): out = (7/2, 7/4, 7).
      (1, 1): h = (7, 2, 8): red > 6 is clipped to 6, green and blue inside: c = col(5) = (5, 5/2, 10): out = (11/2, 9/4, 9).
      (2, 1): h = (1, 1/2, 2): all three below lo: hk = (2, 1, 4), c = col(2): out = (2, 1, 4).
      (3, 1): h = (6, 3, 12) = hi exactly: h > hi is false, untouched: c = col(1): out = (7/2, 7/4, 7).
      (1, 3): h = (5, 7/2, 2): green > 3 -> 3, blue < 4 -> 4, red inside: c = col(5): out = (5, 11/4, 7).
    gamma = 1/2, boxes [3, 5], [3/2, 5/2], [6, 10]: (1, 1): red -> 5: out = (5, 9/4, 9); (3, 1): (6, 3, 12) -> (5, 5/2, 10): out = (3, 3/2, 6).
    gamma = 0: hk = mu = (4, 2, 8) wherever h differs: (1, 1): out = col(9/2) = mean(col(5), col(4)); (0, 1): h = mu already, not clipped.
    gamma = +inf: e = +inf, lo = -inf, hi = +inf: nothing is clipped, (1, 1): out = mean(col(5), (7, 2, 8)) = (6, 9/4, 9).
    min_taps = 16 = S0: the box stands (S0 >= min_taps); min_taps = 17: S0 is one below, hk = h everywhere as with gamma = +inf."""
    a = K(paint(Step(4, 4, cam(0, 0), 4), HISTORY), "variance", gamma, min_taps)
    b = K(Step(4, 4, cam(-1, 0), q), "variance", gamma, min_taps)
    mu, sd = (4, 2, 8), (2, 1, 4)
    g = None if gamma == INF or min_taps > 16 else F(gamma)
    want, clipped = {}, {}
    for (y, x), h in HISTORY.items():
        hk = tuple(F(v) if g is None else min(max(F(v), m - g * s), m + g * s) for v, m, s in zip(h, mu, sd))
        want[(y, x + 1)] = (mean(col(q(y, x + 1)), hk), HALF, 8)
        clipped[(y, x + 1)] = int(hk != tuple(F(v) for v in h))
    want[(2, 0)], clipped[(2, 0)] = (col(2), V0, 4), 0
    if gamma == 1.0 and min_taps <= 16:  # the numbers of the text above
        assert want[(0, 1)][0] == (F(7, 2), F(7, 4), 7) and want[(1, 1)][0] == (F(11, 2), F(9, 4), 9) and want[(2, 1)][0] == (2, 1, 4)
        assert want[(3, 1)][0] == (F(7, 2), F(7, 4), 7) and want[(1, 3)][0] == (5, F(11, 4), 7)
        assert clipped == {(0, 1): 0, (1, 1): 1, (2, 1): 1, (3, 1): 0, (1, 3): 1, (2, 0): 0}
    if gamma == 0.5:
        assert want[(1, 1)][0] == (5, F(9, 4), 9) and want[(3, 1)][0] == (3, F(3, 2), 6)
    if gamma == 0.0:
        assert want[(1, 1)][0] == col(F(9, 2)) and clipped[(0, 1)] == 0 and clipped[(1, 1)] == 1
    if g is None:
        assert want[(1, 1)][0] == (6, F(9, 4), 9) and not any(clipped.values())
    return ClipCase(name or f"clip-box-gamma-{gamma}", box.__doc__, [a, b], want, clipped)


def refused(how):
    """5x4: the box frame in columns 0 .. 3 and a column 4 of colour 100 that is another surface — by its index 9, or by its normal
    (0, 0, -1), dot = -1 < 1/2.  No pixel of columns 0 .. 3 accepts it: their sums are the box frame's 16 taps, and (1, 1) gives
    (11/2, 9/4, 9) as in the 4x4 frame.  Accepted, the five 100s of a row-1 pixel would give mu > 20 and leave h = 7 unclipped."""
    a = K(paint(Step(5, 4, cam(0, 0), 4), HISTORY))
    b = K(Step(5, 4, cam(-1, 0), q))
    for s in (a, b):
        if how == "index":
            s.index[:, 4] = 9
        else:
            s.normal[:, 4] = (0, 0, -1)
    want = {(1, 1): ((F(11, 2), F(9, 4), 9), HALF, 8), (0, 1): ((F(7, 2), F(7, 4), 7), HALF, 8)}
    return ClipCase(f"clip-refused-by-{how}", refused.__doc__, [a, b], want, {(1, 1): 1, (0, 1): 0})


def sky(mode):
    """5x4: columns 0 .. 3 are background with the box frame's colours, column 4 is a hit of colour 100.  History col(4) but (1, 1) =
    (7, 2, 8) through cam(0, 0), then Q through cam(1, 0): a background pixel takes the record to its RIGHT.  ACCUMULATE: the sky pixel
    (1, 0) accepts the 16 misses of its window and not the hits of column 4: boxes [2, 6], [1, 3], [4, 12], h = (7, 2, 8) -> (6, 2, 8),
    c = col(5): out = (11/2, 9/4, 9), V0/2, N = 8.  (0, 0): h = col(4) inside: out = mean(col(3), col(4)).  INPUT: a background pixel
    has no history: out = in = col(5), V0, 4, not clipped."""
    sky_px = [(y, x) for y in range(4) for x in range(4)]
    a = K(paint(Step(5, 4, cam(0, 0), 4), {(1, 1): (7, 2, 8)}), mode=mode, bg=sky_px)
    b = K(Step(5, 4, cam(1, 0), q), mode=mode, bg=sky_px)
    if mode == "accumulate":
        want = {(1, 0): ((F(11, 2), F(9, 4), 9), HALF, 8), (0, 0): (mean(col(3), col(4)), HALF, 8)}
        clipped = {(1, 0): 1, (0, 0): 0}
    else:
        want, clipped = {(1, 0): (col(5), V0, 4)}, {(1, 0): 0}
    return ClipCase(f"clip-sky-{mode}", sky.__doc__, [a, b], want, clipped)


def static_step():
    """The ghost's two frames through ONE camera: a static step is the OFF step, c_out = fma(1/2, 0 - 1, 1) = 1/2 per unit, not 0: a still
    camera keeps converging to the running mean.  Its map is all 0."""
    steps = [K(Step(5, 4, cam(0, 0), 1)), K(Step(5, 4, cam(0, 0), 0))]
    return ClipCase("clip-static", static_step.__doc__, steps, {(1, 2): (col(F(1, 2)), HALF, 8), (0, 0): (col(F(1, 2)), HALF, 8)},
                    {(1, 2): 0, (0, 0): 0})


def cases():
    return [ghost("variance"), ghost("off"), box(1.0), box(0.5), box(0.0), box(INF), box(1.0, 16.0, "clip-min-taps-at"),
            box(1.0, 17.0, "clip-min-taps-below"), refused("index"), refused("normal"), sky("accumulate"), sky("input"), static_step()]


# ---- the moments handle -----------------------------------------------------------------------------------------------------------
def moments_one_frame():
    """4x4, the default w2_max = 1/4.  History col(4) but (1, 0) = (7, 2, 8) through cam(0, 0) — a first frame: m2 = c², W2 = 1 —, then Q
    through cam(-1, 0), gamma = 1.  Pixel (1, 1): h = (7, 2, 8), hq = (49, 4, 64); red is clipped to 6: t = 49 - 49 = 0, hq' = fma(6, 6, 0)
    = 36; green and blue keep hq.  c = col(5) = (5, 5/2, 10): c_out = (11/2, 9/4, 9), m2' = ((25 + 36)/2, (25/4 + 4)/2, (100 + 64)/2);
    W2 = fma(1/4, 1, 1/4) = 1/2 > 1/4: the spatial estimate, from the SAME sums: vn·W2 = (4, 1, 16)/2 = (2, 1/2, 8).  N = 8.
    Pixel (0, 1): unclipped, c_out = mean(col(3), col(4)), the same variance."""
    a = K(paint(MStep(4, 4, cam(0, 0), 4), {(1, 0): (7, 2, 8)}))
    b = K(MStep(4, 4, cam(-1, 0), q))
    v = (2, F(1, 2), 8)
    want = {(1, 1): ((F(11, 2), F(9, 4), 9), v, 8, F(1, 2)), (0, 1): (mean(col(3), col(4)), v, 8, F(1, 2))}
    return ClipMCase("clip-moments-one-frame", moments_one_frame.__doc__, [a, b], want, {(1, 1): 1, (0, 1): 0})


def moments_shift(gamma=1.0):
    """4x4, w2_max = 1/2.  Two STATIC frames on a VARIANCE handle (each the OFF step): col(4) twice, but (1, 0) = (6, 1, 6) then
    (8, 3, 10): c = (7, 2, 8), m2 = ((36 + 64)/2, (1 + 9)/2, (36 + 100)/2) = (50, 5, 68), N = 8, W2 = 1/2; the spread t = m2 - c² =
    (1, 1, 4).  Then Q with 8 samples through cam(-1, 0): hN = 8, Ns = 16, al = k = 1/2.  Pixel (1, 1), gamma = 1: red 7 > 6 is clipped to
    6 and hq' = fma(6, 6, 1) = 37 — the spread stays; green and blue keep hq = 5 and 68.  c = (5, 5/2, 10): c_out = (11/2, 9/4, 9),
    m2' = ((25 + 37)/2, (25/4 + 5)/2, (100 + 68)/2) = (31, 45/8, 84); W2 = fma(1/4, 1/2, 1/4) = 3/8, not > 1/2: the temporal estimate,
    e = (31 - 121/4, 45/8 - 81/16, 84 - 81) = (3/4, 9/16, 3), v = r32(r32(e·3/8) / (5/8)).  N = 16.  Unshifted, red would report
    m2' = (25 + 50)/2 and e = 29/4.  gamma = +inf: nothing clipped, c_out = (6, 9/4, 9), m2' = (75/2, 45/8, 84), e = (3/2, 9/16, 3)."""
    first = K(paint(MStep(4, 4, cam(0, 0), 4, w2_max=0.5), {(1, 0): (6, 1, 6)}), gamma=gamma)
    second = K(paint(MStep(4, 4, cam(0, 0), 4, w2_max=0.5), {(1, 0): (8, 3, 10)}), gamma=gamma)
    third = K(MStep(4, 4, cam(-1, 0), q, spp=8, w2_max=0.5), gamma=gamma)
    if gamma == INF:
        cc, e = (6, F(9, 4), 9), (F(3, 2), F(9, 16), 3)
    else:
        cc, e = (F(11, 2), F(9, 4), 9), (F(3, 4), F(9, 16), 3)
    v = tuple(clamp(r32(r32(x * F(3, 8)) / F(5, 8))) for x in e)
    want = {(1, 1): (cc, v, 16, F(3, 8))}
    return ClipMCase(f"clip-moments-shift-gamma-{gamma}", moments_shift.__doc__, [first, second, third], want, {(1, 1): int(gamma != INF)})


def moments_sky():
    """The plain sky case on a moments handle in ACCUMULATE mode, w2_max = 1/2: (1, 0): h = (7, 2, 8) -> (6, 2, 8), hq = (49, 4, 64) ->
    (36, 4, 64): c_out = (11/2, 9/4, 9), m2' = (61/2, 41/8, 82), W2 = 1/2 not > 1/2: the temporal estimate (a background pixel takes no
    other), e = (61/2 - 121/4, 41/8 - 81/16, 82 - 81) = (1/4, 1/16, 1), v = (e·1/2)/(1/2) = e.  N = 8."""
    sky_px = [(y, x) for y in range(4) for x in range(4)]
    a = K(paint(MStep(5, 4, cam(0, 0), 4, w2_max=0.5), {(1, 1): (7, 2, 8)}), mode="accumulate", bg=sky_px)
    b = K(MStep(5, 4, cam(1, 0), q, w2_max=0.5), mode="accumulate", bg=sky_px)
    want = {(1, 0): ((F(11, 2), F(9, 4), 9), (F(1, 4), F(1, 16), 1), 8, F(1, 2))}
    return ClipMCase("clip-moments-sky", moments_sky.__doc__, [a, b], want, {(1, 0): 1})


def moments_cases():
    return [moments_one_frame(), moments_shift(1.0), moments_shift(INF), moments_sky()]
