"""Hand-derived exact answers for temporal accumulation's moments mode, shared by its CPU and GPU tests.

The frames are tests/temporal_cases.py's: the plane z = 0 through the exact camera `cam(ox, oy)`, every hit with index 7 and the
normal (0, 0, 1) unless a case says otherwise, colours col(a) = (a, a/2, 2a) — so a channel's values are the red channel's times a
power of two, and its variance the red one's times 1/4 or 4, exactly.

A case is a list of steps and, for its LAST step, `want`: {(y, x): (colour, variance, length, W2)} as rationals that ARE f32 values,
each written out in the case from §4.16's formulas with `r32` (one correct rounding, decided in rationals) applied where the
contract rounds.  `spatial` is step 4 in rationals for a list of accepted tap values, which every case that uses it names one by
one."""
from fractions import Fraction as F

import numpy as np

from denoise_cases import R
from temporal_cases import WIDE, Step, cam, col, r32

VCAP = F(2) ** 32
CAP3 = (VCAP, VCAP, VCAP)
MWIDE = dict(WIDE, w2_max=0.25, min_taps=4.0)


def clamp(t):
    return VCAP if not t < VCAP else (t if t > 0 else F(0))


def spatial(values, W2=F(1), mt=F(4)):
    """§4.16 step 4 for ONE channel in rationals: `values`, the accepted taps' colours in tap order.  S0, S1 and S2 are sums the
    cases keep exact (asserted); mu, S2/S0, mu·mu, the difference, dp·S0, the quotient and the product by W2 are rounded as the
    contract rounds them."""
    S0, S1, S2 = F(0), F(0), F(0)
    for v in values:
        S0, S1, S2 = S0 + 1, R(S1 + F(v), "S1"), R(S2 + F(v) * F(v), "S2")
    if S0 < mt:
        return VCAP
    mu = r32(S1 / S0)
    d = r32(r32(S2 / S0) - r32(mu * mu))
    dp = d if d > 0 else F(0)
    return clamp(r32(r32(r32(dp * S0) / (S0 - 1)) * W2))


def spatial3(bases, W2=F(1), mt=F(4)):
    """.. for the three channels of col(a), a in `bases`."""
    return tuple(spatial([col(a)[ch] for a in bases], W2, mt) for ch in range(3))


class MStep(Step):
    def __init__(self, w, h, camera, base, spp=4, reset_before=False, **params):
        super().__init__(w, h, camera, base, spp=spp, reset_before=reset_before)
        self.params = {**MWIDE, **params}


class MCase:
    def __init__(self, name, why, steps, want):
        self.name, self.why, self.steps = name, why, steps
        self.want = {p: (tuple(R(F(c), "colour") for c in cv), tuple(R(F(v), "variance") for v in vv), R(F(N), "length"), R(F(W), "W2"))
                     for p, (cv, vv, N, W) in want.items()}

    def run(self, handle, step_fn):
        """Feeds the steps to `handle` through step_fn(handle, step) -> (rgb, var, length, w2); returns the last step's outputs."""
        out = None
        for s in self.steps:
            if s.reset_before:
                handle.reset()
            out = step_fn(handle, s)
        return out

    def check(self, rgb, var, length, w2, what=""):
        def same(got, want, kind, p):
            w32 = np.float32(float(want))
            assert got.view(np.uint32) == w32.view(np.uint32), f"{self.name} {what}: pixel {p} {kind}: got {got!r}, want {w32!r} ({self.why})"

        for p, (cv, vv, N, W) in self.want.items():
            for ch in range(3):
                same(rgb[p][ch], cv[ch], f"colour {ch}", p)
                same(var[p][ch], vv[ch], f"variance {ch}", p)
            same(length[p], N, "length", p)
            same(w2[p], W, "W2", p)


def one_pixel():
    """A 1x1 first frame, col(3/4): no history, so c_out = c, N = spp = 4, m2 = c·c = (9/16, 9/64, 9/4), W2 = 1 > w2_max = 1/4: the
    spatial estimate, whose only tap is the centre: S0 = 1 < min_taps = 4: v = 2^32."""
    return MCase("one-pixel", one_pixel.__doc__, [MStep(1, 1, cam(), F(3, 4))], {(0, 0): (col(F(3, 4)), CAP3, 4, 1)})


def _ramp(y, x):
    return F(x, 8)


def seven_by_seven():
    """A 7x7 first frame of one surface, base x/8 (red: 0, 1/8 .. 6/8 along every row).  The centre (3, 3) sees all 49 taps: S1 = 7·21/8 =
    147/8, mu = 3/8; S2 = 7·91/64 = 637/64, S2/S0 = 13/64; d = 13/64 − 9/64 = 1/16; (d·49)/48 = 49/768, rounded once; W2 = 1.  The corner
    (0, 0) sees the 16 taps x, y in 0..3: S1 = 3, mu = 3/16, S2 = 7/8, S2/S0 = 7/128, d = 14/256 − 9/256 = 5/256, (d·16)/15 = 1/48,
    rounded once.  (6, 3): x in 0..6, y in 3..6: 28 taps, mu = 3/8, S2/S0 = 13/64 again, d = 1/16, (d·28)/27 = 7/108."""
    s = MStep(7, 7, cam(), _ramp)
    centre = spatial3([_ramp(y, x) for y in range(7) for x in range(7)])
    corner = spatial3([_ramp(y, x) for y in range(4) for x in range(4)])
    edge = spatial3([_ramp(y, x) for y in range(3, 7) for x in range(7)])
    assert centre[0] == r32(F(49, 768)) and corner[0] == r32(F(1, 48)) and edge[0] == r32(F(7, 108))
    assert centre[1] == centre[0] / 4 and centre[2] == centre[0] * 4  # the channels are exact scalings
    want = {(3, 3): (col(F(3, 8)), centre, 4, 1), (0, 0): (col(0), corner, 4, 1), (6, 3): (col(F(3, 8)), edge, 4, 1)}
    return MCase("seven-by-seven", seven_by_seven.__doc__, [s], want)


def refuse_one(how):
    """The 7x7 ramp again, pixel (3, 3).  By index: the tap (2, 5) has index 9 — 48 taps, the value 5/8 missing.  By normal: the tap
    (2, 5) has the normal (0, 0, -1), dot = -1 < 1/2 — the same 48.  By the frame's edge: the pixel (3, 2) instead, whose column
    x = -1 is outside: the 42 taps x in 0..5."""
    s = MStep(7, 7, cam(), _ramp)
    if how == "edge":
        p, taps = (3, 2), [_ramp(y, x) for y in range(7) for x in range(6)]
    else:
        p, taps = (3, 3), [_ramp(y, x) for y in range(7) for x in range(7) if (y, x) != (2, 5)]
        if how == "index":
            s.index[2, 5] = 9
        else:
            s.normal[2, 5] = (0, 0, -1)
    assert len(taps) == (42 if how == "edge" else 48)
    return MCase(f"refuse-one-by-{how}", refuse_one.__doc__, [s], {p: (col(_ramp(*p)), spatial3(taps), 4, 1)})


def centre_always_counts():
    """normal_cos_min = 1 and a centre normal of (0, 0, 1/2): dot(n, n) = 1/4 < 1 would refuse the centre itself, and every other tap
    (dot = 1/2); the centre counts all the same: S0 = 1 < 4: 2^32.  With min_taps = 2 in a 2x1 frame of normals (0, 0, 1) and values
    1/8, 3/8: two taps, mu = 1/4, S2/S0 = 5/64, d = 1/64, (d·2)/1 = 1/32."""
    a = MStep(3, 3, cam(), _ramp, normal_cos_min=1.0)
    a.normal[1, 1] = (0, 0, 0.5)
    b = MStep(2, 1, cam(), lambda y, x: F(1 + 2 * x, 8), min_taps=2.0)
    two = spatial3([F(1, 8), F(3, 8)], mt=F(2))
    assert two[0] == F(1, 32)
    return [MCase("centre-always-counts", centre_always_counts.__doc__, [a], {(1, 1): (col(F(1, 8)), CAP3, 4, 1)}),
            MCase("two-taps", centre_always_counts.__doc__, [b], {(0, 0): (col(F(1, 8)), two, 4, 1), (0, 1): (col(F(3, 8)), two, 4, 1)})]


def background_pixel():
    """A background pixel (index -1): v = +0 whatever its neighbourhood, c_out = c, N = spp, W2 = 1; and its neighbour (0, 0) does not
    count it as a tap: 3x2 frame of base (1 + x + 4y)/8, (0, 1) background: the 5 taps 1/8, 3/8, 5/8, 6/8, 7/8."""
    base = lambda y, x: F(1 + x + 4 * y, 8)  # noqa: E731
    s = MStep(3, 2, cam(), base).background(0, 1)
    taps = [base(y, x) for y in range(2) for x in range(3) if (y, x) != (0, 1)]
    return MCase("background", background_pixel.__doc__, [s], {(0, 1): (col(F(2, 8)), (0, 0, 0), 4, 1), (0, 0): (col(F(1, 8)), spatial3(taps), 4, 1)})


def static_two():
    """Two static frames of 4 spp, alpha_min = 0, w2_max = 1/2, colours col(1) then col(3): hN = 4, Ns = 8, al = k = 1/2; red:
    c_out = 2, m2 = fma(1/2, 9 − 1, 1) = 5, W2 = fma(1/4, 1, 1/4) = 1/2, which is not > 1/2: the temporal estimate, e = 5 − 4 = 1,
    v = (1·1/2) / (1 − 1/2) = 1 = (3 − 1)²/4; green (1/2, 3/2): 1/4; blue (2, 6): 4.  N = 8."""
    steps = [MStep(3, 2, cam(), 1, w2_max=0.5), MStep(3, 2, cam(), 3, w2_max=0.5)]
    want = {p: (col(2), (1, F(1, 4), 4), 8, F(1, 2)) for p in ((0, 0), (1, 2))}
    return MCase("static-two", static_two.__doc__, steps, want)


def static_three():
    """.. and a third frame col(5): hN = 8, Ns = 12, al = r32(1/3), k = r32(1 − al); c_out = fma(al, 5 − 2, 2), m2 = fma(al, 25 − 5, 5),
    W2 = fma(r32(k·k), 1/2, r32(al·al)) — 1/3 to within the roundings, below w2_max = 1/2 —; v = r32(r32(max(m2 − r32(c_out²), 0)·W2) /
    r32(1 − W2)): the variance of the mean of 1, 3, 5 — (4/3)·... = sample variance 4 over 3 frames = 4/3 — to within the roundings."""
    steps = [MStep(3, 2, cam(), a, w2_max=0.5) for a in (1, 3, 5)]
    al = r32(F(4) / 12)
    k = r32(1 - al)
    W2 = r32(r32(k * k) * F(1, 2) + r32(al * al))
    cc, vv = [], []
    for ch in range(3):
        c, h, q = col(5)[ch], col(2)[ch], (5, F(5, 4), 20)[ch]
        co = r32(al * r32(c - h) + h)
        m2 = r32(al * r32(r32(c * c) - q) + q)
        e = r32(m2 - r32(co * co))
        cc.append(co)
        vv.append(clamp(r32(r32((e if e > 0 else 0) * W2) / r32(1 - W2))))
    assert abs(W2 - F(1, 3)) < F(1, 2 ** 22) and abs(vv[0] - F(4, 3)) < F(1, 2 ** 18) and abs(cc[0] - 3) < F(1, 2 ** 21)
    return MCase("static-three", static_three.__doc__, steps, {(0, 0): (tuple(cc), tuple(vv), 12, W2), (1, 1): (tuple(cc), tuple(vv), 12, W2)})


def first_frame_w2_max_one():
    """w2_max = 1 on a first frame: W2 = 1 is not > 1, so step 3 is taken: e = c·c − c·c = 0, (0·1) / (1 − 1) = 0/0 = NaN, which clamps to
    2^32."""
    return MCase("w2-max-one", first_frame_w2_max_one.__doc__, [MStep(7, 7, cam(), _ramp, w2_max=1.0)],
                 {(3, 3): (col(F(3, 8)), CAP3, 4, 1), (0, 0): (col(0), CAP3, 4, 1)})


def w2_max_zero():
    """w2_max = 0: W2 > 0 always, so every step takes the spatial estimate.  Static, a constant first frame col(3/8), then the 7x7 ramp:
    al = k = 1/2, W2 = 1/2, c_out = (3/8 + x/8)/2; the centre's spatial estimate is seven-by-seven's r32(49/768) times W2 = 1/2 —
    a power of two, exact."""
    steps = [MStep(7, 7, cam(), F(3, 8), w2_max=0.0), MStep(7, 7, cam(), _ramp, w2_max=0.0)]
    v = spatial3([_ramp(y, x) for y in range(7) for x in range(7)], W2=F(1, 2))
    assert v[0] == r32(F(49, 768)) / 2
    return MCase("w2-max-zero", w2_max_zero.__doc__, steps, {(3, 3): (col(F(3, 8)), v, 8, F(1, 2)),
                                                             (3, 5): (col(F(1, 2)), spatial3([_ramp(y, x) for y in range(7) for x in range(2, 7)], W2=F(1, 2)), 8, F(1, 2))})


def half_shift():
    """The history moves by half a pixel in x (px_origin by -1/2): taps (px − 1, py) and (px, py) with b = 1/2 each.  First frame col(1)
    everywhere (m2 = 1, W2 = 1), second col(3), alpha_min = 0, w2_max = 1/2: Q = 1/2 + 1/2 = 1, HW = 1, B = 1 — the interpolation of
    equal records is the record — and the blend is static-two's: c_out = 2, W2 = 1/2, v = (1, 1/4, 4), N = 8.  At px = 0 the tap at
    -1 is outside: B = 1/2, Q/B = 1, HW/B = 1: the same."""
    steps = [MStep(4, 3, cam(0, 0), 1, w2_max=0.5), MStep(4, 3, cam(F(-1, 2), 0), 3, w2_max=0.5)]
    return MCase("half-shift", half_shift.__doc__, steps, {p: (col(2), (1, F(1, 4), 4), 8, F(1, 2)) for p in ((0, 0), (1, 2), (2, 3))})


def reset_case():
    """Two static steps, rayz_hip_temporal_reset, the 7x7 ramp: a first frame again — W2 = 1, N = 4, seven-by-seven's spatial estimate."""
    steps = [MStep(7, 7, cam(), 1), MStep(7, 7, cam(), 3), MStep(7, 7, cam(), _ramp, reset_before=True)]
    centre = spatial3([_ramp(y, x) for y in range(7) for x in range(7)])
    return MCase("reset", reset_case.__doc__, steps, {(3, 3): (col(F(3, 8)), centre, 4, 1)})


def cases():
    return ([one_pixel(), seven_by_seven()] + [refuse_one(how) for how in ("index", "normal", "edge")] + centre_always_counts()
            + [background_pixel(), static_two(), static_three(), first_frame_w2_max_one(), w2_max_zero(), half_shift(), reset_case()])
