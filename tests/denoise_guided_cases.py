"""Hand-derived exact answers for the variance-guided denoiser, shared by its CPU and GPU tests.

Every case has FLAT guides — all hits share the normal (0, 0, 1) and lie on the plane z = 0 at P = (x, y, 0), so wn = 1, pl = 0,
u = 1, wz = 1 and g = 1 exactly; a background pixel has NaN colour, and a background-versus-hit tap is skipped — so that what is
left of a tap is exactly what §4.13 adds: the variance prefilter, `den`, the colour weight and the variance sum.  Colours, variances
and sigmas are dyadic.  `exact()` is §4.13 in `fractions.Fraction` on such a frame.  As tests/denoise_cases.py it emulates no f32
step: it REFUSES an intermediate f32 could not hold — here by marking the pixel unknown (None), which every pixel that reads it
inherits — with two absorptions that §4.13 itself states and that are decided by rational comparison:
  * gv + vf = gv where vf is below half an ulp of gv (2^32 + 2^-20 = 2^32);
  * 1 + x = 1 where x = de2 / den <= 2^-24 (round to nearest, ties to even): the colour weight is then 1 to the last bit.
A level's output is one rounded divide per value, so the last level's S / W and V / (W·W) are returned unrounded and rounded ONCE.
Each case also carries `hand`: the closed forms of its docstring at a few pixels, to which the CPU test holds `exact()`."""
from fractions import Fraction as F

import numpy as np

from denoise_cases import K, R, representable, round_f32

ALBEDO = 1
INF = float("inf")
NAN = float("nan")
GK = {-1: F(1, 4), 0: F(1, 2), 1: F(1, 4)}
VCAP = F(2) ** 32


def _rep(x):
    return x if x is not None and representable(x) else None


def pack_v(case):
    """§4.13's pack pass for the variance slot, per pixel: a Fraction (VCAP for a NaN, an infinity or t >= 2^32)."""
    h, w = case.index.shape
    out = {}
    for y in range(h):
        for x in range(w):
            bg = case.index[y, x] < 0
            m = [F(1)] * 3
            if case.params["flags"] & ALBEDO and not bg:
                m = [max(F(float(a)), F(1, 256)) for a in case.albedo[y, x]]
            var = [float(v) for v in case.var_rgb[y, x]]
            if not all(np.isfinite(var)):
                s = sum(np.float32(v) for v in var)  # only to tell -inf from NaN / +inf: no finite arithmetic involved
                out[(y, x)] = F(0) if s == -np.inf else VCAP
                continue
            t = [R(R(F(v), "var") / R(mm * mm, "m.m"), "var / m^2") for v, mm in zip(var, m)]
            t = R(R(t[0] + t[1], "t") + t[2], "t")
            out[(y, x)] = VCAP if not t < VCAP else (t if t > 0 else F(0))
    return out


def exact(case):
    """{pixel: ([3 Fractions], Fraction)}: the last level's S_ch / W and V / (W·W) before their one rounding, for every HIT pixel whose
    value is known (see the module docstring); the colour is still demodulated."""
    prm = case.params
    index = case.index
    h, w = index.shape
    assert (case.normal[index >= 0] == (0, 0, 1)).all() and (case.point[..., 2] == 0).all(), "exact() is for flat guides only"
    sc2 = None if prm["sigma_color"] == INF else R(F(float(np.float32(prm["sigma_color"]))) ** 2, "sc2")
    vf = F(float(np.float32(prm["var_floor"])))
    hit = lambda p: index[p] >= 0  # noqa: E731
    pix = [(y, x) for y in range(h) for x in range(w)]
    v0 = pack_v(case)
    state = {}
    for p in pix:
        if hit(p):
            m = [max(F(float(a)), F(1, 256)) for a in case.albedo[p]] if prm["flags"] & ALBEDO else [F(1)] * 3
            e = [_rep(F(float(c)) / mm) for c, mm in zip(case.rgb[p], m)]
            state[p] = None if None in e else (e, v0[p])
        else:
            state[p] = None  # a background pixel's colour (NaN here) is never read by a hit
    for l in range(prm["levels"]):
        s, nxt, last = 2 ** l, {}, l + 1 == prm["levels"]
        for p in pix:
            nxt[p] = None
            if not hit(p) or state[p] is None:
                continue
            ep, _ = state[p]
            G = A = F(0)
            known = True
            for j in (-1, 0, 1):
                for i in (-1, 0, 1):
                    q = (p[0] + j, p[1] + i)
                    if not (0 <= q[0] < h and 0 <= q[1] < w) or not hit(q):
                        continue
                    if state[q] is None:
                        known = False
                        continue
                    G += GK[i] * GK[j]
                    A = _rep(A + GK[i] * GK[j] * state[q][1]) if A is not None else None
            gv = _rep(A / G) if known and A is not None else None
            if gv is None:
                continue
            if sc2 is not None:
                sum_ = gv + vf
                if not representable(sum_):
                    r = F(float(round_f32(sum_)))
                    if r != gv:
                        continue
                    sum_ = r
                den = _rep(sc2 * sum_)
                if den is None:
                    continue
            W, S, V = F(0), [F(0)] * 3, F(0)
            for j in range(-2, 3):
                for i in range(-2, 3):
                    q = (p[0] + j * s, p[1] + i * s)
                    if not (0 <= q[0] < h and 0 <= q[1] < w) or not hit(q):
                        continue
                    if state[q] is None:
                        known = False
                        break
                    eq, vq = state[q]
                    wc = F(1)
                    if sc2 is not None:
                        de2 = sum((a - b) ** 2 for a, b in zip(eq, ep))
                        x = _rep(de2 / den) if representable(de2) else None
                        if x is None:
                            known = False
                            break
                        one = F(1) if x <= F(1, 2 ** 24) else _rep(1 + x)
                        wc = _rep(1 / one) if one is not None else None
                        if wc is None:
                            known = False
                            break
                    wt = K[i] * K[j] * wc
                    W, V = W + wt, V + wt * wt * vq
                    S = [a + wt * c for a, c in zip(S, eq)]
                    if not all(representable(z) for z in (wt, wt * wt, W, V, *S)):
                        known = False
                        break
                if not known:
                    break
            if not known or not representable(W * W):
                continue
            col, var = [a / W for a in S], V / (W * W)
            if last:
                nxt[p] = (col, var)
            elif all(representable(z) for z in (*col, var)):
                nxt[p] = (col, var)
        state = nxt
    return {p: v for p, v in state.items() if v is not None}


class Case:
    def __init__(self, name, why, rgb, var_rgb, index, albedo, params, hand):
        h, w = index.shape
        self.name, self.why = name, why
        self.rgb, self.var_rgb, self.index, self.albedo = (None if a is None else np.ascontiguousarray(a) for a in (rgb, var_rgb, index, albedo))
        self.normal = np.zeros((h, w, 3), np.float32)
        self.normal[index >= 0] = (0, 0, 1)
        self.point = np.zeros((h, w, 3), np.float32)
        self.point[..., 0], self.point[..., 1] = np.meshgrid(np.arange(w), np.arange(h))
        self.point[index < 0] = 0
        self.params = {**dict(levels=1, normal_power_log2=6, flags=0, sigma_color=INF, sigma_plane=0.25, var_floor=2.0 ** -20), **params}
        self.hand = hand  # {pixel: ([3 Fractions], Fraction)}: S / W and V / (W·W) before their rounding, from the docstring

    def want(self):
        """{pixel: (3 f32, f32)}: every known pixel's output — the one rounding, then ×m (a power of two here, so exact)."""
        out = {}
        for p, (col, var) in exact(self).items():
            m = [max(F(float(a)), F(1, 256)) for a in self.albedo[p]] if self.params["flags"] & ALBEDO else [F(1)] * 3
            out[p] = (tuple(np.float32(float(R(F(float(round_f32(c))) * mm, "out·m"))) for c, mm in zip(col, m)), round_f32(var))
        return out

    def check(self, rgb, var, what=""):
        """`rgb` (h, w, 3) and `var` (h, w) equal the rational expectation bit for bit at every known pixel; every hand pixel is known."""
        want = self.want()
        assert set(self.hand) <= set(want), (self.name, sorted(set(self.hand) - set(want)))
        for p, (c3, v) in want.items():
            for ch in range(3):
                assert rgb[p][ch].view(np.uint32) == c3[ch].view(np.uint32), \
                    f"{self.name} {what}: pixel {p} channel {ch}: got {rgb[p][ch]!r}, want {c3[ch]!r} ({self.why})"
            if var is not None:
                assert var[p].view(np.uint32) == v.view(np.uint32), f"{self.name} {what}: pixel {p} variance: got {var[p]!r}, want {v!r} ({self.why})"


def _field(w, h, colour, var):
    index = np.arange(w * h, dtype=np.int32).reshape(h, w)
    rgb = np.empty((h, w, 3), np.float32)
    rgb[:] = colour
    var_rgb = np.empty((h, w, 3), np.float32)
    var_rgb[:] = var
    return rgb, var_rgb, index


E = [F(1, 2), F(1, 4), F(1)]  # the constant demodulated colour of the uniform cases
SK2 = F(1225, 16384)           # Σ h² over all 25 taps = (Σ k²)² = (35/128)²


def uniform(levels):
    """Uniform variance, demodulated: albedo (1/2, 1/4, 1) everywhere, so m² = (1/4, 1/16, 1); var = (1/32, 1/128, 1/4) gives
    t = (1/8 + 1/8) + 1/4 = 1/2 = v at every pixel; radiance c = e·m with e = (1/2, 1/4, 1) constant.  sigma_color = +inf: den = +inf,
    de2 / den = 0, wc = 1; g = 1: w = h.
    One level, 7x7.  An interior pixel (3, 3) has all 25 taps: W = (Σ k)² = 1, S = e, and V = v·Σ h² = v·(Σ k²)² = v·(35/128)²:
    var_out = v·1225/16384 and the colour is unchanged.  The corner (0, 0) keeps the taps with i, j >= 0: Σ_{i>=0} k = 3/8 + 1/4 + 1/16 =
    11/16, so W = 121/256 and S / W = e; Σ_{i>=0} k² = 9/64 + 1/16 + 1/256 = 53/256, so V = v·2809/65536 and
    var_out = v·(2809/65536) / (121/256)² = v·2809/14641, one rounded divide.
    Two levels, 13x13.  Every pixel at least 2 from the border leaves level 0 with variance v·1225/16384 and colour e; pixel (6, 6)
    reads, at stride 2, pixels 2..10 only — all of those — so it leaves level 1 with v·(1225/16384)²."""
    n = 7 if levels == 1 else 13
    m = np.array([0.5, 0.25, 1.0], np.float32)
    rgb, var_rgb, index = _field(n, n, np.array([float(x) for x in E], np.float32) * m, (1 / 32, 1 / 128, 1 / 4))
    albedo = np.empty((n, n, 3), np.float32)
    albedo[:] = m
    v = F(1, 2)
    if levels == 1:
        hand = {(3, 3): (E, v * SK2), (0, 0): (E, v * F(2809, 14641)), (6, 0): (E, v * F(2809, 14641))}
    else:
        hand = {(6, 6): (E, v * SK2 * SK2)}
    return Case(f"uniform-L{levels}", uniform.__doc__, rgb, var_rgb, index, albedo, dict(levels=levels, flags=ALBEDO), hand)


def _step(var, sigma_color):
    rgb, var_rgb, index = _field(5, 5, 0.0, var)
    rgb[:, 3:] = 1.0
    return rgb, var_rgb, index, dict(sigma_color=sigma_color)


def step_v0():
    """A 0/1 colour step, 5x5: e = (0,0,0) for x <= 2, (1,1,1) for x >= 3; v = 0 everywhere, var_floor = 2^-20, sigma_color = 1024, one
    level.  gv = 0 / G = 0; den = sc2·(0 + vf) = 2^20·2^-20 = 1.  Across the edge de2 = 3: wc = 1 / (1 + 3/1) = 1/4; on one side
    de2 = 0, wc = 1.  The column sums of h are k[i] (Σ_j k[j] = 1).  Pixel (2, 2), e_p = 0, all 25 taps: i = -2..0 on its side,
    i = 1, 2 across: W = (1/16 + 1/4 + 3/8) + (1/4 + 1/16)/4 = 11/16 + 5/64 = 49/64, S = 5/64: out = 5/49.  Pixel (2, 3), e_p = 1:
    i = 2 is outside the frame, i = -2, -1 across: W = (1/16 + 1/4)/4 + (3/8 + 1/4) = 5/64 + 40/64 = 45/64, S = 40/64: out = 8/9.
    Every v is 0: var_out = 0 / W² = 0."""
    rgb, var_rgb, index, prm = _step(0.0, 1024.0)
    hand = {(2, 2): ([F(5, 49)] * 3, F(0)), (2, 3): ([F(8, 9)] * 3, F(0))}
    return Case("step-v0", step_v0.__doc__, rgb, var_rgb, index, None, prm, hand)


def step_vcap():
    """The same step with var = +inf, so v = VCAP = 2^32 everywhere, sigma_color = 1: gv = (G·2^32) / G = 2^32, gv + vf = 2^32 + 2^-20 =
    2^32 (absorbed), den = 2^32; across the edge x = de2 / den = 3·2^-32.  wc = 1 TO THE LAST BIT whenever x <= 2^-24, because 1 + x
    then rounds to 1 (at x = 2^-24 the tie goes to the even neighbour, 1): with v = VCAP that is de2 <= 2^8·sc2, here 3 <= 256.  So the
    level is the plain 5x5 B-spline: pixel (2, 2) has W = 1 and S = k[1] + k[2] = 5/16; pixel (2, 3): W = 15/16 (i = 2 outside),
    S = 3/8 + 1/4 = 5/8, out = 2/3.  var_out = 2^32·Σ h² / W²: (2, 2): 2^32·1225/16384 = 1225·2^18; (2, 3): the columns i = -2..1 have
    Σ k² = 1/256 + 1/16 + 9/64 + 1/16 = 69/256 and the rows 35/128: V = 2^32·(69/256)(35/128), var_out = V / (15/16)²."""
    rgb, var_rgb, index, prm = _step(INF, 1.0)
    hand = {(2, 2): ([F(5, 16)] * 3, VCAP * SK2), (2, 3): ([F(2, 3)] * 3, VCAP * F(69, 256) * F(35, 128) / F(225, 256))}
    return Case("step-vcap", step_vcap.__doc__, rgb, var_rgb, index, None, prm, hand)


def background_neighbour():
    """The prefilter skips a background pixel.  3x3, one level; (1, 2) is background with NaN colour and var = +inf (v = VCAP); every
    hit has var = (1/4, 1/8, 1/8): v = 1/2.  var_floor = 1/2, sigma_color = 1.  At p = (1, 1) the prefilter has gg = 1/4 at the centre,
    1/8 at an edge neighbour, 1/16 at a corner; without (1, 2): G = 1 - 1/8 = 7/8, A = 7/16, gv = 1/2 (with it, gv would be about
    2^29 and every wc 1).  den = 1·(1/2 + 1/2) = 1.  e = (1,1,1) at (0, 1) and 0 elsewhere: that tap has de2 = 3, wc = 1/4, h = k[0]·k[-1] =
    3/32, w = 3/128.  The other hit taps (±2 is outside a 3x3 frame): centre 9/64, edges (2, 1) and (1, 0) 3/32 each, four corners
    1/16 each; (1, 2) is skipped.  W = 9/64 + 12/64 + 16/64 + 3/128 = 77/128, S = 3/128: out = 3/77.
    V = (1/2)·(81/4096 + 2·9/1024 + 4·1/256 + 9/16384) = (1/2)·877/16384; var_out = (877/32768) / (77/128)² = 877/11858."""
    rgb, var_rgb, index = _field(3, 3, 0.0, (1 / 4, 1 / 8, 1 / 8))
    rgb[0, 1] = 1.0
    index[1, 2] = -1
    rgb[1, 2] = NAN
    var_rgb[1, 2] = INF
    hand = {(1, 1): ([F(3, 77)] * 3, F(877, 11858))}
    return Case("background-neighbour", background_neighbour.__doc__, rgb, var_rgb, index, None, dict(sigma_color=1.0, var_floor=0.5), hand)


def cases():
    return [uniform(1), uniform(2), step_v0(), step_vcap(), background_neighbour()]


def odd_variances():
    """One pixel of a 5x5 uniform field (v = 1/2, constant colour 1/2) gets a NaN, a +inf or a negative variance in its red channel:
    its packed v is VCAP, VCAP and 0.  Returns [(label, case, pixel, the pixel's v)]; the outputs must hold no NaN."""
    out = []
    for label, bad, v in (("nan", NAN, VCAP), ("+inf", INF, VCAP), ("negative", -4.0, F(0))):
        rgb, var_rgb, index = _field(5, 5, 0.5, (1 / 4, 1 / 8, 1 / 8))
        var_rgb[2, 2, 0] = bad
        out.append((label, Case(f"odd-variance-{label}", odd_variances.__doc__, rgb, var_rgb, index, None, dict(levels=2, sigma_color=2.0), {}),
                    (2, 2), v))
    return out


def guided_variance(rgb, seed):
    """A per-channel variance for synthetic frames: spanning 0, tiny, ordinary and large values, with +inf, NaN and negative entries."""
    rng = np.random.default_rng(seed)
    var = (rgb * rgb * 10.0 ** rng.uniform(-6, 1, rgb.shape)).astype(np.float32)
    kind = rng.random(rgb.shape)
    var[kind < 0.04] = 0
    var[(kind >= 0.04) & (kind < 0.06)] = 1e-30
    var[(kind >= 0.06) & (kind < 0.08)] = 1e12
    var[(kind >= 0.08) & (kind < 0.10)] = np.inf
    var[(kind >= 0.10) & (kind < 0.12)] = np.nan
    var[(kind >= 0.12) & (kind < 0.13)] = -1.0
    return var
