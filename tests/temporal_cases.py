"""Hand-derived exact answers for temporal accumulation, shared by its CPU and GPU tests.

The exact camera.  `cam(ox, oy)` has px_du = (1, 0, 0), px_dv = (0, 1, 0), px_origin = (ox, oy, 0), look_from = (0, 0, -8): a = (ox, oy, 8),
v×a = (8, 0, -ox), a×u = (0, 8, -oy), u×v = (0, 0, 1), det = 8, so M = [[1, 0, -ox/8], [0, 1, -oy/8], [0, 0, 1/8]] — exact in f32 for
the small integers and dyadic fractions used here.  A point (X, Y, 0) has w = (X, Y, 8), gamma = 1, alpha = X - ox, beta = Y - oy.
The scene is the plane z = 0: the pixel (px, py) of a frame made with cam(ox, oy) sees P = (px + ox, py + oy, 0), so in the previous
frame, made with cam(ox', oy'), it lay at x = px + ox - ox', y = py + oy - oy': moving px_origin by (-k, 0, 0) moves the history k
pixels to the right.  All hits share index 7 and the normal (0, 0, 1) unless a case says otherwise; colours are (a, a/2, 2a).

A case is a list of steps and, for its LAST step, `want`: {(y, x): (colour, variance, length)} as rationals that ARE f32 values — each
written out in the case from §4.15's formulas, with `r32` (one correct rounding, decided in rationals) applied exactly where the
contract rounds and nowhere else.  Every other value of a derivation is exact, which `R` asserts."""
from fractions import Fraction as F

import numpy as np

from denoise_cases import R, round_f32

INF = float("inf")
NAN = float("nan")
VCAP = F(2) ** 32
WIDE = dict(alpha_min=0.0, n_max=INF, normal_cos_min=0.5, max_rel_dist=0.25)  # r2 = 1/16: lim = ww/16 >= 4, far above a pixel's 1/2


def r32(x):
    return F(float(round_f32(F(x))))


def cam(ox=0, oy=0, fz=-8):
    return dict(look_from=(0.0, 0.0, float(fz)), px_du=(1.0, 0.0, 0.0), px_dv=(0.0, 1.0, 0.0), px_origin=(float(ox), float(oy), 0.0))


def col(a):
    a = F(a)
    return (a, a / 2, 2 * a)


class Step:
    def __init__(self, w, h, camera, base, var=(F(1, 4), F(1, 8), F(1, 2)), spp=4, reset_before=False, **params):
        """A frame of the plane through `camera`: colour col(base[y][x]) (base: a function of (y, x) or a constant), variance `var`
        everywhere (three values or a function of (y, x))."""
        self.camera, self.spp, self.reset_before = camera, spp, reset_before
        self.params = {**WIDE, **params}
        ox, oy = camera["px_origin"][0], camera["px_origin"][1]
        self.index = np.full((h, w), 7, np.int32)
        self.normal = np.zeros((h, w, 3), np.float32)
        self.normal[..., 2] = 1
        gx, gy = np.meshgrid(np.arange(w), np.arange(h))
        self.point = np.stack([gx + ox, gy + oy, np.zeros((h, w))], axis=2).astype(np.float32)
        self.rgb = np.empty((h, w, 3), np.float32)
        self.var = np.empty((h, w, 3), np.float32)
        for y in range(h):
            for x in range(w):
                self.rgb[y, x] = [float(c) for c in col(base(y, x) if callable(base) else base)]
                self.var[y, x] = [float(c) for c in (var(y, x) if callable(var) else var)]

    def background(self, y, x):
        self.index[y, x] = -1
        self.normal[y, x] = 0
        self.point[y, x] = 0
        return self


class Case:
    def __init__(self, name, why, steps, want):
        self.name, self.why, self.steps = name, why, steps
        self.want = {p: (tuple(R(F(c), "colour") for c in cv), tuple(R(F(v), "variance") for v in vv), R(F(N), "length"))
                     for p, (cv, vv, N) in want.items()}

    def run(self, handle, step_fn):
        """Feeds the steps to `handle` through step_fn(handle, step) -> (rgb, var, length); returns the last step's outputs."""
        out = None
        for s in self.steps:
            if s.reset_before:
                handle.reset()
            out = step_fn(handle, s)
        return out

    def check(self, rgb, var, length, what=""):
        for p, (cv, vv, N) in self.want.items():
            for ch in range(3):
                for got, w_, kind in ((rgb[p][ch], cv[ch], "colour"), (var[p][ch], vv[ch], "variance")):
                    w32 = np.float32(float(w_))
                    assert got.view(np.uint32) == w32.view(np.uint32), \
                        f"{self.name} {what}: pixel {p} {kind} {ch}: got {got!r}, want {w32!r} ({self.why})"
            w32 = np.float32(float(N))
            assert length[p].view(np.uint32) == w32.view(np.uint32), f"{self.name} {what}: pixel {p} length: got {length[p]!r}, want {w32!r}"


V0 = (F(1, 4), F(1, 8), F(1, 2))  # the default variance of a Step


def blend(c, s, h, hv, hN, spp, am=F(0), nm=None):
    """§4.15 step 4 in rationals, `r32` at every operation the contract performs (the identity wherever the value is exact)."""
    Ns = r32(hN + spp)
    a0 = r32(F(spp) / Ns)
    al = am if a0 < am else a0
    k = r32(1 - al)
    a2, k2 = r32(al * al), r32(k * k)
    cc = tuple(r32(al * r32(ci - hi) + hi) for ci, hi in zip(c, h))
    vv = tuple(r32(a2 * si + r32(k2 * hvi)) for si, hvi in zip(s, hv))
    N = Ns if nm is None or not Ns > nm else nm
    return cc, vv, N


def first_frame():
    """One step on a fresh handle: no history, so out = in by selection, N = spp = 4.  The variance is clamped as §4.13's pack clamps:
    (1/4, +inf, NaN) -> (1/4, 2^32, 2^32) at (0, 0); (-1, 0, 2^40) -> (0, 0, 2^32) at (0, 1)."""
    var = lambda y, x: {(0, 0): (0.25, INF, NAN), (0, 1): (-1.0, 0.0, 2.0 ** 40)}.get((y, x), V0)  # noqa: E731
    s = Step(3, 2, cam(), lambda y, x: F(1 + x + 4 * y, 8), var=var)
    want = {(0, 0): (col(F(1, 8)), (F(1, 4), VCAP, VCAP), 4), (0, 1): (col(F(2, 8)), (0, 0, VCAP), 4), (1, 2): (col(F(7, 8)), V0, 4)}
    return Case("first-frame", first_frame.__doc__, [s], want)


def static_two():
    """Static camera, two steps of 4 spp, colours col(1) then col(3), variance V0 both: hN = 4, Ns = 8, a0 = 1/2, c = fma(1/2, 3 - 1, 1)
    = 2 (per channel: the mean), k = 1/2, v = 1/4·s + 1/4·s = s/2, N = 8."""
    steps = [Step(3, 2, cam(), 1), Step(3, 2, cam(), 3)]
    want = {p: (col(2), tuple(v / 2 for v in V0), 8) for p in ((0, 0), (1, 2))}
    return Case("static-two", static_two.__doc__, steps, want)


def static_three():
    """.. and a third step with col(6): h = col(2), hv = V0/2, hN = 8, Ns = 12, a0 = r32(4/12) — 1/3 is rounded HERE and only here as a
    quotient; c = r32(a0·(6 - 2) + 2) per channel (c - h exact), k = r32(1 - a0), v = r32(r32(a0²)·s + r32(r32(k²)·s/2)), N = 12.  The
    running mean (1 + 3 + 6)/3 = 10/3 to within those roundings."""
    steps = [Step(3, 2, cam(), 1), Step(3, 2, cam(), 3), Step(3, 2, cam(), 6)]
    w = blend(col(6), V0, col(2), tuple(v / 2 for v in V0), 8, 4)
    assert w[2] == 12 and abs(w[0][0] - F(10, 3)) < F(1, 2 ** 21) and abs(w[1][0] - V0[0] / 3) < F(1, 2 ** 24)
    return Case("static-three", static_three.__doc__, steps, {(0, 0): w, (1, 1): w})


def shift(kx, ky):
    """px_origin moves by (-kx, -ky): the pixel (px, py) lay at (px - kx, py - ky), x0 = px - kx, fx = 0: the tap (x0, y0) has b = 1, the other
    three b = 0 (accepted or outside alike: + 0).  History base (1 + x + 8y)/16 per pixel, current colour 0: out = h/2, v = V0/2, N = 8
    where px >= kx and py >= ky; in the uncovered strip x = px - kx <= -1 fails `x > -1`: no history, out = 0, v = V0, N = 4."""
    w, h = 5, 4
    base = lambda y, x: F(1 + x + 8 * y, 16)  # noqa: E731
    steps = [Step(w, h, cam(0, 0), base), Step(w, h, cam(-kx, -ky), 0)]
    want = {}
    for y in range(h):
        for x in range(w):
            if x >= kx and y >= ky:
                want[(y, x)] = (tuple(c / 2 for c in col(base(y - ky, x - kx))), tuple(v / 2 for v in V0), 8)
            else:
                want[(y, x)] = (col(0), V0, 4)
    return Case(f"shift-{kx}-{ky}", shift.__doc__, steps, want)


def half_shift(both):
    """px_origin moves by (-1/2, 0) (or (-1/2, -1/2)): x = px - 1/2, x0 = px - 1, fx = 1/2.  One axis: taps (px-1, py) and (px, py) with b = 1/2
    each, the j = 1 taps b = 0.  History base (x + 4y)/8, current 0: h = (base(px-1) + base(px))/2, out = h/2.  Both axes: four taps of
    b = 1/4.  At px = 0 the tap at -1 is outside: B = 1/2 (both axes, at the corner: 1/4), h = H / B = base(0, ..) renormalised — exact
    divides by powers of two.  v = V0/2 (all taps share V0), N = 8."""
    w, h = 4, 3
    base = lambda y, x: F(x + 4 * y, 8)  # noqa: E731
    steps = [Step(w, h, cam(0, 0), base), Step(w, h, cam(F(-1, 2), F(-1, 2) if both else 0), 0)]
    want = {}
    for y in range(h):
        for x in range(w):
            xs = [q for q in (x - 1, x) if q >= 0]
            ys = [q for q in ((y - 1, y) if both else (y,)) if q >= 0]
            hb = sum(base(yy, xx) for yy in ys for xx in xs) / (len(xs) * len(ys))
            want[(y, x)] = (tuple(c / 2 for c in col(hb)), tuple(v / 2 for v in V0), 8)
    return Case("half-shift-xy" if both else "half-shift-x", half_shift.__doc__, steps, want)


def refuse_one(how):
    """Half-pixel shift on both axes, 3x3; the pixel (1, 1) has the taps (0,0), (0,1), (1,0), (1,1) of b = 1/4.  History bases 1, 2, 4, 8
    there; the tap (0, 1) (base 2) is refused — by its index (9), by its normal ((0,0,-1): dot = -1 < 1/2) or by its distance (its point
    lifted to z = 4: |d|² = 1/2 + 16 > lim = (1/16)·(1/4 + 1/4 + 64) = 4 + 1/32, P = (1/2, 1/2, 0); the others have |d|² = 1/2).  B = 3/4, H = (1 + 4 + 8)/4 = 13/4,
    h = r32((13/4) / (3/4)) = r32(13/3) per unit of colour — the renormalisation, one rounded divide; current colour 0:
    out = fma(1/2, -h, h) = h/2.  hv = r32((3/4·s) / (3/4)) = s, v = s/2; hN = 4, N = 8."""
    base = {(0, 0): 1, (0, 1): 2, (1, 0): 4, (1, 1): 8}
    a = Step(3, 3, cam(0, 0), lambda y, x: base.get((y, x), 16))
    if how == "id":
        a.index[0, 1] = 9
    elif how == "normal":
        a.normal[0, 1] = (0, 0, -1)
    else:
        a.point[0, 1, 2] = 4
    b = Step(3, 3, cam(F(-1, 2), F(-1, 2)), 0)
    hc = tuple(r32(R(F(13, 4) * u, "H") / F(3, 4)) for u in (1, F(1, 2), 2))
    want = {(1, 1): (tuple(c / 2 for c in hc), tuple(v / 2 for v in V0), 8)}
    return Case(f"refuse-one-by-{how}", refuse_one.__doc__, [a, b], want)


def refuse_all():
    """The same with all four history pixels of index 9: no tap accepted, B = 0 is not >= 2^-6: no history, out = in = col(1/2), N = 4."""
    a = Step(3, 3, cam(0, 0), 1)
    a.index[:] = 9
    b = Step(3, 3, cam(F(-1, 2), F(-1, 2)), F(1, 2))
    return Case("refuse-all", refuse_all.__doc__, [a, b], {(1, 1): (col(F(1, 2)), V0, 4), (0, 0): (col(F(1, 2)), V0, 4)})


def weight_threshold(at):
    """px_origin moves by (+1/8, +fy): x = px + 1/8, x0 = px, fx = 1/8; the tap (px+1, py+1) has b = fx·fy, and it is the only one accepted
    (every other history pixel has index 9).  fy = 1/8: b = B = 2^-6, which IS >= 2^-6: h = (b·c)/b = c exactly, history col(3),
    current col(1): out = col(2), N = 8.  fy = 127/1024: b = 127/8192 < 2^-6: no history, out = col(1), N = 4.  Pixel (0, 0), tap (1, 1)."""
    a = Step(3, 3, cam(0, 0), 3)
    a.index[:] = 9
    a.index[1, 1] = 7
    b = Step(3, 3, cam(F(1, 8), F(1, 8) if at else F(127, 1024)), 1)
    want = {(0, 0): (col(2), tuple(v / 2 for v in V0), 8) if at else (col(1), V0, 4)}
    return Case("weight-at-2^-6" if at else "weight-below-2^-6", weight_threshold.__doc__, [a, b], want)


def background_pixel():
    """Static, two steps; (0, 1) is background (index -1) in the SECOND frame only: out = in there, N = 4, although the history pixel is
    a hit; (1, 1) is background in the FIRST frame only: its record has index -1, which equals no id >= 0: no history either.  (0, 0)
    blends as static-two."""
    a = Step(3, 2, cam(), 1).background(1, 1)
    b = Step(3, 2, cam(), 3).background(0, 1)
    want = {(0, 1): (col(3), V0, 4), (1, 1): (col(3), V0, 4), (0, 0): (col(2), tuple(v / 2 for v in V0), 8)}
    return Case("background", background_pixel.__doc__, [a, b], want)


def behind_camera():
    """One-pixel shift; the current frame's pixel (0, 2) reports a point at z = -16, behind the previous camera (look_from z = -8):
    w_z = -8, gamma = (1/8)·(-8) = -1 is not > 0: the projection fails, out = in = col(1/2), N = 4.  At (0, 3) the point lies ON the
    camera plane (z = -8): gamma = 0, not > 0 either.  (0, 1) follows its history: h = col(base(0, 0)) = col(1), out = fma(1/2, 1/2 - 1, 1) = 3/4."""
    a = Step(4, 1, cam(0, 0), lambda y, x: 1 + x)
    b = Step(4, 1, cam(-1, 0), F(1, 2))
    b.point[0, 2, 2] = -16
    b.point[0, 3, 2] = -8
    want = {(0, 2): (col(F(1, 2)), V0, 4), (0, 3): (col(F(1, 2)), V0, 4), (0, 1): (col(F(3, 4)), tuple(v / 2 for v in V0), 8)}
    return Case("behind-camera", behind_camera.__doc__, [a, b], want)


def alpha_min_binds():
    """static-two with alpha_min = 3/4: a0 = 1/2 < 3/4, al = 3/4: c = fma(3/4, 3 - 1, 1) = 5/2 per unit, k = 1/4,
    v = 9/16·s + 1/16·s = 5/8·s, N = 8."""
    steps = [Step(3, 2, cam(), 1), Step(3, 2, cam(), 3, alpha_min=0.75)]
    want = {(0, 0): (col(F(5, 2)), tuple(v * F(5, 8) for v in V0), 8)}
    return Case("alpha-min-binds", alpha_min_binds.__doc__, steps, want)


def n_max_binds():
    """static, n_max = 6: step 2 has Ns = 8 > 6, N = 6 (colour as static-two: 2).  Step 3 with col(7): hN = 6, Ns = 10, a0 = r32(4/10),
    c = r32(a0·(7 - 2) + 2), N = min(10, 6) = 6 — the history never outweighs 6 samples."""
    steps = [Step(3, 2, cam(), 1, n_max=6.0), Step(3, 2, cam(), 3, n_max=6.0), Step(3, 2, cam(), 7, n_max=6.0)]
    w = blend(col(7), V0, col(2), tuple(v / 2 for v in V0), 6, 4, nm=F(6))
    assert w[2] == 6 and abs(w[0][0] - 4) < F(1, 2 ** 20)
    return Case("n-max-binds", n_max_binds.__doc__, steps, {(1, 2): w})


def odd_variances():
    """static, two steps; variances per pixel (first frame -> second frame), red channel (green and blue are V0's):
    (0,0): +inf -> 1/4: hv = 2^32, v = 1/16 + 2^30;   (0,1): NaN -> +inf: v = 2^30 + 2^30 = 2^31;   (0,2): -1 -> 0: v = 0;
    (1,0): 0 -> NaN: v = 2^30;   (1,1): 1/4 -> -inf: s = 0, v = 1/16;   (1,2): 2^40 -> 2^-30: v = r32(2^-32 + 2^30) = 2^30.
    Colours col(1), col(3): col(2), N = 8; nothing is NaN."""
    v1 = {(0, 0): INF, (0, 1): NAN, (0, 2): -1.0, (1, 0): 0.0, (1, 1): 0.25, (1, 2): 2.0 ** 40}
    v2 = {(0, 0): 0.25, (0, 1): INF, (0, 2): 0.0, (1, 0): NAN, (1, 1): -INF, (1, 2): 2.0 ** -30}
    steps = [Step(3, 2, cam(), 1, var=lambda y, x: (v1[(y, x)], 0.125, 0.5)), Step(3, 2, cam(), 3, var=lambda y, x: (v2[(y, x)], 0.125, 0.5))]
    red = {(0, 0): F(1, 16) + F(2) ** 30, (0, 1): F(2) ** 31, (0, 2): 0, (1, 0): F(2) ** 30, (1, 1): F(1, 16), (1, 2): F(2) ** 30}
    want = {p: (col(2), (r32(r), V0[1] / 2, V0[2] / 2), 8) for p, r in red.items()}
    return Case("odd-variances", odd_variances.__doc__, steps, want)


def reset_case():
    """Two static steps, rayz_hip_temporal_reset, a third step: a first frame again — out = in = col(5), v = V0, N = 4."""
    steps = [Step(3, 2, cam(), 1), Step(3, 2, cam(), 3), Step(3, 2, cam(), 5, reset_before=True)]
    return Case("reset", reset_case.__doc__, steps, {(0, 0): (col(5), V0, 4), (1, 2): (col(5), V0, 4)})


def cases():
    out = [first_frame(), static_two(), static_three()]
    out += [shift(kx, ky) for kx, ky in ((1, 0), (2, 0), (0, 1), (0, 2), (1, 1), (2, 2), (2, 1))]
    out += [half_shift(False), half_shift(True)]
    out += [refuse_one(how) for how in ("id", "normal", "distance")]
    out += [refuse_all(), weight_threshold(True), weight_threshold(False), background_pixel(), behind_camera(), alpha_min_binds(),
            n_max_binds(), odd_variances(), reset_case()]
    return out


# ---- sequences on synthetic guides (the CPU and GPU tests feed the same ones to the mirror and to the device) ------------------
def plane_sequence(w, h, seed, origins, margin=3):
    """Frames of ONE synthetic world seen through exact cameras cam(ox, oy): tests/denoise_cases.py's `synthetic` guides on a canvas
    `margin` cells larger on every side, the world point of canvas cell (X, Y) being (X, Y, 0).  The pixel (px, py) of a frame sees the
    point (px + ox, py + oy, 0) exactly and takes index and normal from the canvas cell nearest to it, so integer origins give frames
    that are windows of one field and fractional ones frames whose taps agree with some neighbours and not with others.  Colour and
    variance are drawn afresh per frame (variances spanning 0, tiny, large, +inf and NaN).  Returns a list of dicts."""
    from denoise_cases import synthetic
    from denoise_guided_cases import guided_variance

    _, index, normal, _, _ = synthetic(w + 2 * margin, h + 2 * margin, seed)
    gx, gy = np.meshgrid(np.arange(w), np.arange(h))
    frames = []
    for k, (ox, oy) in enumerate(origins):
        assert abs(ox) <= margin - 1 and abs(oy) <= margin - 1
        cx = np.floor(gx + ox + 0.5).astype(int) + margin
        cy = np.floor(gy + oy + 0.5).astype(int) + margin
        idx, nrm = index[cy, cx].copy(), normal[cy, cx].copy()
        pt = np.stack([gx + ox, gy + oy, np.zeros((h, w))], axis=2).astype(np.float32)
        pt[idx < 0] = 0
        rgb = synthetic(w, h, seed + 101 * (k + 1))[0]
        frames.append(dict(rgb=rgb, var=guided_variance(rgb, seed + k), index=np.ascontiguousarray(idx), normal=np.ascontiguousarray(nrm),
                           point=pt, camera=cam(ox, oy)))
    return frames


def general_sequence(w, h, seed, shifts=((0.0, 0.0), (0.0, 0.0), (1.37, 0.61))):
    """Three frames through a general camera whose arithmetic is NOT exact — first, the same camera again (static), then a pan of
    (1.37, 0.61) pixels (`shifts`: each frame's pan from the first camera, in pixels): the world is the plane z = 5 + x/10, every point the f32 of the f64 intersection of its pixel's ray; the
    hittable index is constant over blocks of 6x4 pixels, `synthetic`'s normals and background."""
    from denoise_cases import synthetic
    from denoise_guided_cases import guided_variance

    u, v = np.array([0.0123, 0.0004, -0.0007]), np.array([0.0003, -0.0119, 0.0011])
    lf = np.array([0.3, 1.7, -6.1])
    po0 = lf + np.array([0.0, 0.0, 1.0]) - u * (w / 2) - v * (h / 2)
    gx, gy = np.meshgrid(np.arange(w), np.arange(h))
    frames = []
    for k, shift in enumerate(shifts):
        po = po0 + shift[0] * u + shift[1] * v
        d = (po - lf)[None, None, :] + gx[..., None] * u + gy[..., None] * v
        t = (5.0 + 0.1 * lf[0] - lf[2]) / (d[..., 2] - 0.1 * d[..., 0])  # z = 5 + x/10 along lf + t·d
        _, idx, nrm, _, _ = synthetic(w, h, seed)
        idx = np.where(idx < 0, -1, gx // 6 + 10 * (gy // 4)).astype(np.int32)  # blocks of one hittable: taps inside agree, across do not
        rgb = synthetic(w, h, seed + 13 * (k + 1))[0]
        pt = (lf[None, None, :] + t[..., None] * d).astype(np.float32)
        pt[idx < 0] = 0
        camera = dict(look_from=tuple(lf), px_du=tuple(u), px_dv=tuple(v), px_origin=tuple(po))
        frames.append(dict(rgb=rgb, var=guided_variance(rgb, seed + k), index=idx, normal=nrm, point=pt, camera=camera))
    return frames


def edge_sequence(w, h, seed):
    """`general_sequence`'s world under pans that put the frame's first column, then its first row, 1/128 of a pixel inside the
    history's border: x = px − 127/128, so at px = 0 the tap at −1 is outside and the tap at 0 has b = 1/128 < 2^-6 — no history, by
    the weight threshold.  A reading that lets the outside tap take the clamped pixel has B = 1 there and blends: at a frame's edge
    the clamped tap and its in-frame neighbour are the same pixel, so B is the ONLY thing such a reading changes."""
    return general_sequence(w, h, seed, shifts=((0.0, 0.0), (-127 / 128, 0.0), (-127 / 128 + 0.25, -127 / 128)))


MOVING_SPP = (4, 8, 16, 8, 4)


def _turned(vecs, yaw, pitch, roll):
    """The vectors turned about the world's y, x and z axes by the three (small) angles."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    R = (np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]])
         @ np.array([[cr, -sr, 0], [sr, cr, 0], [0, 0, 1]]))
    return [R @ x for x in vecs]


def moving_cameras(w, h):
    """Five general cameras over the world of `moving_sequence`: a first one; the same again (a static step); look_from moved
    sideways and forward by a fraction of the scene's depth (about 15); the view turned by a few pixels' worth of angle, a roll
    included, so that px_du, px_dv and px_origin all change; and one more move with a further small turn."""
    u, v, f = np.array([0.0123, 0.0004, -0.0007]), np.array([0.0003, -0.0119, 0.0011]), np.array([0.0, 0.0, 1.0])
    lf = np.array([0.3, 1.7, -6.1])
    poses = [(lf, (u, v, f))] * 2
    lf3 = lf + np.array([0.62, -0.17, 0.55])
    poses.append((lf3, (u, v, f)))
    t4 = _turned((u, v, f), 0.031, -0.017, 0.012)  # a pixel is 0.0123 rad wide
    poses.append((lf3, t4))
    poses.append((lf3 + np.array([-0.33, 0.21, 0.4]), _turned(t4, -0.011, 0.008, -0.004)))
    cams = []
    for o, (uu, vv, ff) in poses:
        po = o + ff - uu * (w / 2) - vv * (h / 2)
        cams.append(dict(look_from=tuple(o), px_du=tuple(uu), px_dv=tuple(vv), px_origin=tuple(po)))
    return cams


def moving_sequence(w, h, seed):
    """Five frames of ONE synthetic world through `moving_cameras`, spp 4, 8, 16, 8, 4 (frame["spp"]).  Two depth layers, about 15
    and 10 from the first camera: the far plane z = 9 + x/10 − y/20 where |x − 0.3| < 0.3·w·0.0123·15 (beyond it is background, so
    the frame has background columns that move with the camera), and in front of it the slab z = 4 + 3y/100 over the world
    rectangle −0.9 < x < 0.5, 0.8 < y < 2.3 — silhouettes, parallax between the layers and disocclusion behind the slab's edges when
    look_from moves.  Every point is the f32 of the f64 intersection of its pixel's ray; index and normal belong to the surface hit
    and are functions of the WORLD position: the index is constant over world cells a few pixels wide (taps inside agree, across do
    not), the normal is the plane's with a ripple that turns it by up to ~0.2 rad between neighbouring pixels (so normal_cos_min =
    0.99 refuses taps that 0.9 accepts) and is NEGATED on stripes of the far plane (a back-facing patch of one hittable: what tells
    `dot >= cm` from `|dot| >= cm`).  Colour and variance are drawn per frame as `general_sequence` draws them."""
    from denoise_cases import synthetic
    from denoise_guided_cases import guided_variance

    gx, gy = np.meshgrid(np.arange(w), np.arange(h))
    planes = [(np.array([-0.1, 0.05, 1.0]), 9.0), (np.array([0.0, -0.03, 1.0]), 4.0)]  # n·X = c
    half_width = 0.3 * w * 0.0123 * 15
    frames = []
    for k, camera in enumerate(moving_cameras(w, h)):
        lf, u, v, po = (np.array(camera[f]) for f in ("look_from", "px_du", "px_dv", "px_origin"))
        d = (po - lf)[None, None, :] + gx[..., None] * u + gy[..., None] * v
        X, hitl = [], []
        for pn, pc in planes:
            t = (pc - pn @ lf) / (d @ pn)
            X.append(lf[None, None, :] + t[..., None] * d)
            hitl.append(t > 0)
        far, slab = X
        on_far = hitl[0] & (np.abs(far[..., 0] - 0.3) < half_width)
        on_slab = hitl[1] & (slab[..., 0] > -0.9) & (slab[..., 0] < 0.5) & (slab[..., 1] > 0.8) & (slab[..., 1] < 2.3)
        pt = np.where(on_slab[..., None], slab, far)
        cell = np.where(on_slab, 300 + np.floor(pt[..., 0] / 0.37) + 10 * np.floor(pt[..., 1] / 0.29),
                        100 + np.floor(pt[..., 0] / 0.83) + 20 * np.floor(pt[..., 1] / 0.61))
        idx = np.where(on_slab | on_far, cell, -1).astype(np.int32)
        base = np.where(on_slab[..., None], -planes[1][0], -planes[0][0])  # facing the camera
        freq = np.where(on_slab, 19.0, 12.0)
        ripple = np.stack([np.sin(freq * pt[..., 0]), np.cos(freq * 0.8 * pt[..., 1] + 0.4), np.zeros((h, w))], axis=2)
        nrm = base + 0.12 * ripple
        nrm /= np.linalg.norm(nrm, axis=2, keepdims=True)
        nrm = np.where((~on_slab & (np.sin(2.3 * pt[..., 0] + 0.7 * pt[..., 1]) > 0.75))[..., None], -nrm, nrm)
        rgb = synthetic(w, h, seed + 13 * (k + 1))[0]
        pt, nrm = pt.astype(np.float32), nrm.astype(np.float32)
        pt[idx < 0] = 0
        nrm[idx < 0] = 0
        frames.append(dict(rgb=rgb, var=guided_variance(rgb, seed + k), index=idx, normal=np.ascontiguousarray(nrm),
                           point=np.ascontiguousarray(pt), camera=camera, spp=MOVING_SPP[k]))
    return frames


def orbit_views():
    """Five (look_from, look_at) pairs around threeSpheres' own view ((-2, 2, 1) towards (0, 0, -1), about 3.5 away, a pixel about
    0.01 rad at 64x36): the first; the same again; an orbit sideways and up with look_at following; a dolly towards the scene; and
    an orbit back with look_at raised — moves of a pixel or two each, with look_from AND look_at changing."""
    return [((-2.0, 2.0, 1.0), (0.0, 0.0, -1.0)), ((-2.0, 2.0, 1.0), (0.0, 0.0, -1.0)), ((-1.94, 2.03, 1.05), (0.02, 0.0, -1.0)),
            ((-1.86, 1.95, 0.97), (0.02, 0.0, -1.0)), ((-1.9, 1.92, 1.04), (0.0, 0.03, -0.98))]


def orbit_camera(oracle, view, w, h):
    """threeSpheres' camera (vfov 20, focus 3.4, no defocus) at a view of `orbit_views`, from the oracle's camera_init."""
    from rayz_amd import capi

    c = capi.CameraDesc()
    oracle.load().rayz_oracle_camera_init(20.0, 3.4, 0.0, capi.D3(*view[0]), capi.D3(*view[1]), capi.D3(0, 1, 0), h, w, c)
    return c
