"""Hand-derived exact answers for temporal accumulation's cubic resampling mode, shared by its CPU and GPU tests,
and the sequence whose index blocks are large enough for the mode to be taken.

The frames are tests/temporal_cases.py's: the plane z = 0 through the exact camera `cam(ox, oy)`, index 7, normal (0, 0, 1), colours
col(a) = (a, a/2, 2a).  A frame made with cam(sx, sy) after one made with cam(0, 0) finds the history of its pixel (px, py) at
(px + sx, py + sy): x0 = px + floor(sx), fx = frac(sx).  All cases are 6x6 and look at the pixel (2, 2) unless they say otherwise:
its window with a shift in [0, 1) is columns and rows 1 .. 4.  The current frame is black with spp = 4 on a history of 4: al = 1/2
and out = fma(1/2, 0 − h, h) = h/2, exactly; v = V0/2; N = 8.

`cubic` is §4.26 in rationals, `r32` (one correct rounding, decided in rationals) at every operation the contract performs."""
from fractions import Fraction as F

import numpy as np

from denoise_cases import R
from temporal_cases import V0, Case, Step, cam, col, r32
from temporal_moments_cases import MCase, MStep

HALF_V0 = tuple(v / 2 for v in V0)
FAR = dict(max_rel_dist=0.5)  # r2 = 1/4: lim = |P − from|²/4 > 16, beyond the window's farthest tap (|d|² < 6); WIDE's 1/16 would refuse the corners


def CStep(*args, **params):
    return Step(*args, **{**FAR, **params})


def weights(f):
    """§4.26's four weights of f, every operation rounded as the contract rounds it."""
    f = F(f)
    f2 = r32(f * f)
    fma = lambda a, b, c: r32(F(a) * F(b) + F(c))  # noqa: E731
    return (r32(f * fma(f, fma(F(-1, 2), f, 1), F(-1, 2))), fma(f2, fma(F(3, 2), f, F(-5, 2)), 1),
            r32(f * fma(f, fma(F(-3, 2), f, 2), F(1, 2))), r32(f2 * fma(F(1, 2), f, F(-1, 2))))


WEIGHTS = {F(0): (0, 1, 0, 0), F(1, 4): (F(-9, 128), F(111, 128), F(29, 128), F(-3, 128)), F(1, 2): (F(-1, 16), F(9, 16), F(9, 16), F(-1, 16)),
           F(3, 4): (F(-3, 128), F(29, 128), F(111, 128), F(-9, 128)), F(1): (0, 0, 1, 0)}  # the exact dyadics


def cubic(taps, fx, fy, divide=True):
    """§4.26's sums, divide and clamp for ONE channel: taps[j][i], j, i = 0 .. 3 standing for −1 .. 2.  (divide False: the misreading
    hc = C, for `divide_case`.)"""
    wx, wy = weights(fx), weights(fy)
    W, C = F(0), F(0)
    for j in range(4):
        for i in range(4):
            b = r32(wx[i] * wy[j])
            W = r32(W + b)
            C = r32(b * F(taps[j][i]) + C)
    hc = r32(C / W) if divide else C
    inner = [F(taps[j][i]) for j in (1, 2) for i in (1, 2)]
    lo, hi = min(inner), max(inner)
    return lo if hc < lo else (hi if hc > hi else hc)


def window(base, y0=2, x0=2):
    return [[base(y0 + j, x0 + i) for i in (-1, 0, 1, 2)] for j in (-1, 0, 1, 2)]


class CubicCase(Case):
    """A Case of a plain handle in cubic mode, plus `taken`: {(y, x): 0 or 1} for the last step."""

    def __init__(self, name, why, steps, want, taken):
        super().__init__(name, why, steps, want)
        self.taken = taken

    def check_taken(self, taken, what=""):
        for p, t in self.taken.items():
            assert taken[p] == t, f"{self.name} {what}: pixel {p} taken: got {taken[p]}, want {t} ({self.why})"


def quad(y, x):
    return F(x * x + 2 * y * y + x + y, 8)


def quadratic(mode):
    """History base (x² + 2y² + x + y)/8, shifted by (1/2, 1/4).  Cubic: Catmull-Rom reproduces a quadratic, and with dyadic weights
    (…/16 and …/128) every product and partial sum is exact in f32, so h is the polynomial at (2.5, 2.25) = 169/64 per unit of
    colour; it increases along both axes, so it lies between the inner taps and the clamp does not bind.  Bilinear: the chord of
    x² over one pixel lies A·fx(1 − fx) above it: h = 169/64 + (1/8)(1/4) + (2/8)(3/16) = 169/64 + 5/64."""
    steps = [CStep(6, 6, cam(0, 0), quad), CStep(6, 6, cam(F(1, 2), F(1, 4)), 0)]
    exact = (F(5, 2) ** 2 + 2 * F(9, 4) ** 2 + F(5, 2) + F(9, 4)) / 8
    assert exact == F(169, 64)
    if mode == "cubic":
        h = cubic(window(quad), F(1, 2), F(1, 4))
        assert h == exact
    else:
        h = exact + F(1, 8) * F(1, 2) * F(1, 2) + F(2, 8) * F(1, 4) * F(3, 4)
        assert h == sum(quad(2 + j, 2 + i) * (F(1, 2)) * (F(1, 4) if j else F(3, 4)) for j in (0, 1) for i in (0, 1))
    want = {(2, 2): (tuple(c / 2 for c in col(h)), HALF_V0, 8)}
    return CubicCase(f"quadratic-{mode}", quadratic.__doc__, steps, want, {(2, 2): int(mode == "cubic"), (0, 0): 0, (4, 4): 0})


def clamp_case(low):
    """Shift (1/2, 0): wy = (0, 1, 0, 0), so only the row y0 counts.  Columns 1 .. 4 hold (1, 0, 0, 1): −1/16 − 1/16 = −1/8, below both
    inner taps: clamped to 0.  Columns (0, 1, 1, 0): 9/16 + 9/16 = 9/8, above both: clamped to 1."""
    row = {1: 1, 4: 1} if low else {2: 1, 3: 1}
    base = lambda y, x: F(row.get(x, 0))  # noqa: E731
    steps = [CStep(6, 6, cam(0, 0), base), CStep(6, 6, cam(F(1, 2), 0), 0)]
    h = cubic(window(base), F(1, 2), 0)
    assert h == (0 if low else 1)
    return CubicCase("clamp-low" if low else "clamp-high", clamp_case.__doc__, steps, {(2, 2): (tuple(c / 2 for c in col(h)), HALF_V0, 8)},
                     {(2, 2): 1})


def integer_shift():
    """px_origin moves by (−1, −1): the pixel lay at (px − 1, py − 1), fx = fy = 0, weights (−0, 1, 0, 0): C = the tap (x0, y0)'s colour
    and W = 1, exactly — the bilinear bits, with taken = 1 at (2, 2) (window 0 .. 3) and taken = 0 at (1, 1), whose window starts at −1."""
    base = lambda y, x: F(1 + x + 8 * y, 16)  # noqa: E731
    steps = [CStep(6, 6, cam(0, 0), base), CStep(6, 6, cam(-1, -1), 0)]
    want = {p: (tuple(c / 2 for c in col(base(p[0] - 1, p[1] - 1))), HALF_V0, 8) for p in ((2, 2), (1, 1), (3, 4))}
    return CubicCase("integer-shift", integer_shift.__doc__, steps, want, {(2, 2): 1, (1, 1): 0, (3, 4): 1, (0, 0): 0})


BASES = {(2, 2): 1, (2, 3): 2, (3, 2): 4, (3, 3): 8}


def outer_refused(how):
    """Shift (1/2, 1/2); the inner taps (2,2), (2,3), (3,2), (3,3) hold 1, 2, 4, 8, every other pixel 16.  The OUTER tap (1, 1) is
    refused — by its index (9), by its normal ((0, 0, −1)) or by its distance (z = 8: |d|² > 64 > lim = 76.5/4) — so the cubic path is not taken and the result is
    the bilinear one: four taps of b = 1/4, h = 15/4."""
    a = CStep(6, 6, cam(0, 0), lambda y, x: BASES.get((y, x), 16))
    if how == "id":
        a.index[1, 1] = 9
    elif how == "normal":
        a.normal[1, 1] = (0, 0, -1)
    else:
        a.point[1, 1, 2] = 8
    steps = [a, CStep(6, 6, cam(F(1, 2), F(1, 2)), 0)]
    return CubicCase(f"outer-refused-by-{how}", outer_refused.__doc__, steps, {(2, 2): (tuple(c / 2 for c in col(F(15, 4))), HALF_V0, 8)},
                     {(2, 2): 0, (3, 3): 1})


def outer_outside():
    """The same frames; the pixel (0, 0) has x0 = y0 = 0, so its window starts at −1, outside the frame: bilinear, four taps of 16."""
    steps = [CStep(6, 6, cam(0, 0), lambda y, x: BASES.get((y, x), 16)), CStep(6, 6, cam(F(1, 2), F(1, 2)), 0)]
    return CubicCase("outer-outside", outer_outside.__doc__, steps, {(0, 0): (tuple(c / 2 for c in col(16)), HALF_V0, 8)}, {(0, 0): 0, (2, 2): 1})


def inner_refused():
    """.. and the INNER tap (2, 3) (base 2) refused by its index: §4.15's renormalised bilinear value, tests/temporal_cases.py's
    refuse_one: B = 3/4, H = 13/4, h = r32((13/4)/(3/4)) per unit of colour."""
    a = CStep(6, 6, cam(0, 0), lambda y, x: BASES.get((y, x), 16))
    a.index[2, 3] = 9
    hc = tuple(r32(R(F(13, 4) * u, "H") / F(3, 4)) for u in (1, F(1, 2), 2))
    return CubicCase("inner-refused", inner_refused.__doc__, [a, CStep(6, 6, cam(F(1, 2), F(1, 2)), 0)],
                     {(2, 2): (tuple(c / 2 for c in hc), HALF_V0, 8)}, {(2, 2): 0})


def divide_case():
    """The quadratic history shifted by (k/1024, k/1024) for the first k from 333 on at which the f32 weights do not sum to 1 and
    hc = C / W differs from C in every channel's last bits: the one place where the division by W shows.  In f64 W is 1 to 1e-16 and
    the two readings agree far inside any bound, so this case, in rationals, is what holds the section's divide."""
    for k in range(333, 400):
        f = F(k, 1024)
        per = [(cubic([[col(v)[ch] for v in row] for row in window(quad)], f, f), cubic([[col(v)[ch] for v in row] for row in window(quad)], f, f, False))
               for ch in range(3)]
        if all(a != b for a, b in per):
            break
    else:
        raise AssertionError("no fraction found at which the divide shows")
    steps = [CStep(6, 6, cam(0, 0), quad), CStep(6, 6, cam(f, f), 0)]
    case = CubicCase("divide", divide_case.__doc__, steps, {(2, 2): (tuple(a / 2 for a, _ in per), HALF_V0, 8)}, {(2, 2): 1})
    case.without_divide = tuple(b / 2 for _, b in per)
    return case


def cases():
    return [divide_case(), quadratic("cubic"), clamp_case(True), clamp_case(False), integer_shift(), outer_refused("id"), outer_refused("normal"),
            outer_refused("distance"), outer_outside(), inner_refused()]


def bilinear_cases():
    """What the same frames give a handle left in bilinear mode (taken = 0 everywhere)."""
    c = quadratic("bilinear")
    return [c]


# ---- the moments step --------------------------------------------------------------------------------------------------------
NEVER_SPATIAL = dict(w2_max=1.0, **FAR)  # W2 > 1 never holds: the variance is step 3's, from the history's m2


def lin(y, x):
    return F(x + 2 * y + 1, 8)


def moments_quadratic():
    """History base (x + 2y + 1)/8 after one frame: m2 = c², a QUADRATIC per channel, shifted by (1/2, 1/4) — both the colour and m2 are
    reproduced exactly: h = (2.5 + 2·2.25 + 1)/8 = 1 per unit of colour at (2.5, 2.25), hq = h² per channel.  Black current frame: c' = h/2, m2' = hq/2,
    W2 = fma(1/4, 1, 1/4) = 1/2, v = (m2' − c'²)·(1/2)/(1/2) = h²/4 per channel."""
    steps = [MStep(6, 6, cam(0, 0), lin, **NEVER_SPATIAL), MStep(6, 6, cam(F(1, 2), F(1, 4)), 0, **NEVER_SPATIAL)]
    want_c, want_v = [], []
    for ch in range(3):
        h = cubic([[col(v)[ch] for v in row] for row in window(lin)], F(1, 2), F(1, 4))
        hq = cubic([[col(v)[ch] ** 2 for v in row] for row in window(lin)], F(1, 2), F(1, 4))
        assert h == col(1)[ch] and hq == h * h
        c2, m2 = h / 2, hq / 2
        e = r32(m2 - r32(c2 * c2))
        want_c.append(c2)
        want_v.append(r32(r32(e * F(1, 2)) / F(1, 2)))
        assert want_v[-1] == h * h / 4
    return MCase("moments-quadratic", moments_quadratic.__doc__, steps, {(2, 2): (tuple(want_c), tuple(want_v), 8, F(1, 2))})


def moments_negative():
    """Shift (1/2, 0), columns 1 .. 4 hold 0, 1, 2, 4: h = (9 + 18 − 4)/16 = 23/16, inside [1, 2]; m2's red row is 0, 1, 4, 16:
    hq = (9 + 36 − 16)/16 = 29/16, inside [1, 4] — and below h² = 529/256: the negative lobes break m2 >= c².  The current frame's
    colour at (2, 2) is col(23/16) = h: c' = h, m2' = (h² + hq)/2 rounded, m2' − c'² = (hq − h²)/2 < 0 in every channel: v = 0."""
    row = {1: 0, 2: 1, 3: 2, 4: 4}
    base = lambda y, x: F(row.get(x, 0))  # noqa: E731
    steps = [MStep(6, 6, cam(0, 0), base, **NEVER_SPATIAL), MStep(6, 6, cam(F(1, 2), 0), F(23, 16), **NEVER_SPATIAL)]
    h = cubic(window(base), F(1, 2), 0)
    hq = cubic([[v * v for v in r] for r in window(base)], F(1, 2), 0)
    assert h == F(23, 16) and hq == F(29, 16) and hq < h * h
    return MCase("moments-negative", moments_negative.__doc__, steps, {(2, 2): (col(h), (0, 0, 0), 8, F(1, 2))})


def moments_cases():
    return [moments_quadratic(), moments_negative()]


# ---- a sequence on which both populations are large ---------------------------------------------------------------------------
def block_sequence(w, h, seed, shifts=((0.0, 0.0), (0.0, 0.0), (1.37, 0.61), (2.12, 1.43)), block=(16, 8)):
    """tests/temporal_cases.py's `general_sequence` — the plane z = 5 + x/10 through a general camera, first, static, a fractional pan
    and a further one — with the hittable index constant over blocks of 16x8 pixels and ONE normal, so that a pixel well inside a
    block has sixteen history taps of its own surface (the cubic path) and one within two pixels of a block's border, of the
    background or of the frame's edge does not (the bilinear fallback): `general_sequence`'s 6x4 blocks leave at most one pixel in
    eight eligible.  The background is `synthetic`'s, thinned to whole blocks."""
    from denoise_cases import synthetic
    from denoise_guided_cases import guided_variance
    from temporal_cases import general_sequence

    frames = general_sequence(w, h, seed, shifts=shifts)
    gx, gy = np.meshgrid(np.arange(w), np.arange(h))
    bx, by = gx // block[0], gy // block[1]
    _, idx0, _, _, _ = synthetic(w, h, seed)
    bg = (idx0[np.minimum(by * block[1], h - 1), np.minimum(bx * block[0], w - 1)] < 0) & ((bx + by) % 3 == 2)
    index = np.where(bg, -1, bx + 10 * by).astype(np.int32)
    normal = np.zeros((h, w, 3), np.float32)
    normal[..., :] = np.array([-0.1, 0.0, 1.0], np.float32) / np.float32(np.sqrt(1.01))
    normal[index < 0] = 0
    for k, f in enumerate(frames):
        f["index"], f["normal"] = index.copy(), normal.copy()
        # (general_sequence zeroed the points of ITS background; the plane's points of this index's hits are recomputed from the camera)
        lf, u, v, po = (np.array(f["camera"][n]) for n in ("look_from", "px_du", "px_dv", "px_origin"))
        d = (po - lf)[None, None, :] + gx[..., None] * u + gy[..., None] * v
        t = (5.0 + 0.1 * lf[0] - lf[2]) / (d[..., 2] - 0.1 * d[..., 0])
        pt = (lf[None, None, :] + t[..., None] * d).astype(np.float32)
        pt[index < 0] = 0
        f["point"] = pt
        f["var"] = guided_variance(f["rgb"], seed + k)
    return frames
