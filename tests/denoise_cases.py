"""Inputs the denoiser's CPU and GPU tests share: the synthetic guides, and small frames whose answers are
EXACT — every quantity dyadic, every intermediate of §4.11 representable in f32 — worked out with `fractions.Fraction` from the
formulas of §4.11 and rounded ONCE, at the final divide.

`exact()` is §4.11 in rational arithmetic for the hit pixels of a tiny frame.  It emulates no f32 step: it computes in exact
rationals and REFUSES (AssertionError) any intermediate that f32 could not hold, which is what makes one final rounding the whole
difference between the rational answer and a conforming f32 evaluation.  Every case also carries `hand`: the closed form of its
docstring, written out with literal weights, which the CPU test holds `exact()` to — so the general evaluator is itself pinned.

The two-pixel construction.  Pixels A and B are hits 2^L apart along a row, a column or a diagonal of a frame run with
`levels = L`; every other pixel is background with NaN colour.  A hit-versus-background tap is skipped, so no NaN may reach a hit, and
A and B meet ONCE, at the last level, through the `±2` tap.  (A frame of width 2^l + 1 run to `levels = l + 1` would NOT isolate
level l: distance 2^l is also reached by level l - 1 through i = ±2.)  At the levels before the last a hit sees only its own centre tap:
W = 9/64·g_c, S = W·e exactly, S / W = e, so the last level starts from the packed colours."""
from fractions import Fraction as F

import numpy as np

ALBEDO = 1  # RAYZ_DENOISE_ALBEDO
INF = float("inf")
K = {-2: F(1, 16), -1: F(1, 4), 0: F(3, 8), 1: F(1, 4), 2: F(1, 16)}
NAN3 = (float("nan"),) * 3


def synthetic(w, h, seed):
    """Guides that exercise every branch of a tap: regions with their own base normal (so wn is 0 across some borders and near 1
    inside), normals and points perturbed pixel by pixel, blocks of background (their normal and point 0, as a query writes them),
    pairs of pixels that share one point exactly (d2 == 0), an albedo with channels below the 2^-8 floor, and a noisy colour."""
    rng = np.random.default_rng(seed)
    gx, gy = np.meshgrid(np.arange(w), np.arange(h))
    region = ((gx // 9) + 2 * (gy // 7)) % 5
    base = rng.normal(size=(5, 3))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    normal = base[region] + rng.normal(scale=0.08, size=(h, w, 3))
    normal /= np.linalg.norm(normal, axis=2, keepdims=True)
    point = np.stack([gx * 0.05, gy * 0.05, region * 0.3], axis=2) + rng.normal(scale=0.004, size=(h, w, 3))
    if w > 1:
        same = rng.random((h, w - 1)) < 0.05
        point[:, 1:][same] = point[:, :-1][same]
    index = rng.integers(0, 400, (h, w)).astype(np.int32)
    bg = ((gx // 11 + gy // 5) % 4 == 0) | (rng.random((h, w)) < 0.03)
    index[bg] = -1
    normal[bg] = 0
    point[bg] = 0
    albedo = rng.random((h, w, 3))
    albedo[rng.random((h, w, 3)) < 0.05] = 0.001
    albedo[bg] = 0
    rgb = np.abs(albedo * (0.8 + 0.4 * np.sin(gx * 0.11 + gy * 0.07))[..., None] + rng.normal(scale=0.3, size=(h, w, 3)))
    rgb[bg] = (0.5, 0.7, 1.0) + rng.normal(scale=0.1, size=(int(bg.sum()), 3))
    f = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    return f(rgb), index, f(normal), f(point), f(albedo)


# ---- exact rational arithmetic ------------------------------------------------------------------------------------------------
def representable(x):
    """Is the rational x a finite f32 (normal or subnormal)?"""
    if x == 0:
        return True
    n, d = abs(x.numerator), x.denominator
    if d & (d - 1):
        return False
    return n.bit_length() - ((n & -n).bit_length() - 1) <= 24 and d <= 2 ** 149 and n < 2 ** 128 * d


def R(x, what=""):
    assert representable(x), f"{what} = {x} is not an f32: the case is not exact"
    return x


def round_f32(x):
    """The rational x correctly rounded to f32 (nearest, ties to even), decided by rational comparison."""
    if x == 0:
        return np.float32(0)
    c = np.float32(float(x))
    cand = (np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf)))
    return min(cand, key=lambda v: (abs(F(float(v)) - x), int(v.view(np.uint32)) & 1))


def _dot(a, b, what):
    """dot(a, b) = fma(a_z, b_z, fma(a_y, b_y, a_x·b_x)): three results, each of which must be an f32."""
    s = R(a[0] * b[0], what)
    s = R(s + a[1] * b[1], what)
    return R(s + a[2] * b[2], what)


def _fr(a):
    return [F(float(v)) for v in a]


def exact(case, weights=None):
    """§4.11 in rationals on the hit pixels of `case`.  Returns {(y, x): three Fractions, the last level's S / W before its one
    rounding, or None where W = 0}; the final ×m is applied by expectation().  Requires that hits never have a finite path to
    a background pixel's colour, which the skip rule guarantees, so background pixels are not evaluated at all.  `weights`, a dict, receives {pixel: the last level's w, tap by tap}."""
    prm = case.params
    index = case.index
    h, w = index.shape
    L, npl = prm["levels"], prm["normal_power_log2"]
    sp2 = R(F(float(np.float32(prm["sigma_plane"]))) ** 2, "sp2")
    sc2 = None if prm["sigma_color"] == INF else R(F(float(np.float32(prm["sigma_color"]))) ** 2, "sc2")
    hits = [(y, x) for y in range(h) for x in range(w) if index[y, x] >= 0]
    n = {p: _fr(case.normal[p]) for p in hits}
    P = {p: _fr(case.point[p]) for p in hits}
    m = modulation(case)
    e = {p: [R(c / mm, "e") for c, mm in zip(_fr(case.rgb[p]), m[p])] for p in hits}
    for l in range(L):
        s, cl, nxt = 2 ** l, F(4) ** l, {}
        for p in hits:
            W, S = F(0), [F(0)] * 3
            for j in range(-2, 3):
                for i in range(-2, 3):
                    q = (p[0] + j * s, p[1] + i * s)
                    if not (0 <= q[0] < h and 0 <= q[1] < w) or index[q] < 0:
                        continue  # outside the frame, or hit versus background: skipped
                    assert e[q] is not None, "a 0/0 pixel is read by a later level: the case must stop at one level"
                    hk = K[i] * K[j]
                    wn = max(F(0), _dot(n[p], n[q], "n.n"))
                    for _ in range(npl):
                        wn = R(wn * wn, "wn")
                    v = [R(a - b, "v") for a, b in zip(P[q], P[p])]
                    d2, pl = _dot(v, v, "d2"), _dot(n[p], v, "pl")
                    wz = F(1)
                    if d2 != 0:
                        u = max(F(0), R(1 - R(R(pl * pl, "pl2") / R(sp2 * d2, "sp2.d2"), "ratio"), "u"))
                        wz = R(u * u, "wz")
                    g = R(wn * wz, "g")
                    if g == 0:
                        wt = F(0)  # (h·0)·wc = 0 for any finite wc, and wc = 1 / (1 + x), x >= 0 finite, is in (0, 1]
                    else:
                        de = [R(a - b, "de") for a, b in zip(e[q], e[p])]
                        x = F(0) if sc2 is None else R(R(_dot(de, de, "de2") * cl, "de2.cl") / sc2, "x")
                        wc = R(1 / R(1 + x, "1+x"), "wc")
                        wt = R(R(hk * g, "h.g") * wc, "w")
                    W = R(W + wt, "W")
                    if weights is not None and l == L - 1:
                        weights.setdefault(p, []).append(wt)
                    S = [R(sc + wt * c, "S") for sc, c in zip(S, e[q])]
            if W == 0:
                nxt[p] = None  # 0 / 0
            else:
                nxt[p] = [sc / W for sc in S] if l == L - 1 else [R(sc / W, "a level's output") for sc in S]
        e = nxt
    return e


def modulation(case):
    """m per hit pixel: max(a, 2^-8) per channel when the case demodulates, else 1."""
    out = {}
    for y, x in zip(*np.nonzero(case.index >= 0)):
        if case.params["flags"] & ALBEDO:
            out[(y, x)] = [max(a, F(1, 256)) for a in _fr(case.albedo[y, x])]
        else:
            out[(y, x)] = [F(1)] * 3
    return out


def expectation(case, values):
    """{pixel: 3 Fractions or None} -> {pixel: 3 f32}: the one rounding of S / W, then ×m, which must be exact (m a power of two)."""
    m = modulation(case)
    out = {}
    for p, v in values.items():
        if v is None:
            out[p] = tuple(np.float32(x) for x in NAN3)
        else:
            out[p] = tuple(np.float32(float(R(F(float(round_f32(c))) * mm, "out·m"))) for c, mm in zip(v, m[p]))
    return out


class Case:
    def __init__(self, name, why, rgb, index, normal, point, albedo, params, hand, general=True):
        self.name, self.why = name, why
        self.rgb, self.index, self.normal, self.point, self.albedo = rgb, index, normal, point, albedo
        self.params = params
        self.hand = hand          # {pixel: 3 Fractions (S / W before its rounding) or None (0 / 0)}: the docstring's closed form
        self.general = general    # False: an intermediate is NOT an f32 (stated in `why`), so exact() does not apply; `hand` stands alone

    def want(self):
        return expectation(self, self.hand)

    def check(self, out, what=""):
        """`out` (h, w, 3) f32 equals the rational expectation bit for bit at every hit pixel (NaN where it says 0 / 0)."""
        for p, w3 in self.want().items():
            got = out[p]
            for c in range(3):
                same = (np.isnan(w3[c]) and np.isnan(got[c])) or got[c].view(np.uint32) == w3[c].view(np.uint32)
                assert same, f"{self.name} {what}: pixel {p} channel {c}: got {got[c]!r}, want {w3[c]!r} ({self.why})"


def mix(c, ep, w, eq):
    """(c·e_p + w·e_q) / (c + w) per channel: a centre tap of weight c and ONE neighbour of weight w."""
    return [(c * a + w * b) / (c + w) for a, b in zip(ep, eq)]


def _v(*x):
    return tuple(F(a) for a in x)


def pair(name, why, L, npl, hand_a, hand_b, axis="row", n_a=(0, 0, 1), n_b=(0, 0, F(1, 2)), P_a=(0, 0, 0), P_b=(1, 0, 1),
         c_a=(0, 0, 0), c_b=(1, 1, 1), a_a=None, a_b=None, sigma_color=None, sigma_plane=1, general=True, span=None):
    """Two hits `span` (default 2^L) pixels apart, NaN background between and around them.  sigma_color defaults to 2^(L-1), so
    that dot(de, de)·4^(L-1) / sc2 = dot(de, de)."""
    d = 2 ** L if span is None else span
    shape = {"row": (1, d + 1), "col": (d + 1, 1), "diag": (d + 1, d + 1)}[axis]
    A, B = (0, 0), {"row": (0, d), "col": (d, 0), "diag": (d, d)}[axis]
    index = np.full(shape, -1, np.int32)
    normal = np.zeros(shape + (3,), np.float32)
    point = np.zeros(shape + (3,), np.float32)
    rgb = np.full(shape + (3,), np.nan, np.float32)
    albedo = None if a_a is None else np.zeros(shape + (3,), np.float32)
    for p, nn, PP, cc, aa, k in ((A, n_a, P_a, c_a, a_a, 7), (B, n_b, P_b, c_b, a_b, 11)):
        index[p], normal[p], point[p], rgb[p] = k, [float(x) for x in nn], [float(x) for x in PP], [float(x) for x in cc]
        if albedo is not None:
            albedo[p] = [float(x) for x in aa]
    params = dict(levels=L, normal_power_log2=npl, flags=0 if albedo is None else ALBEDO,
                  sigma_color=float(2 ** (L - 1)) if sigma_color is None else sigma_color, sigma_plane=float(sigma_plane))
    return Case(name, why, rgb, index, normal, point, albedo, params, {A: hand_a, B: hand_b}, general)


H2, H1, HD, C0 = F(3, 128), F(3, 32), F(1, 256), F(9, 64)  # k[±2]·k[0], k[±1]·k[0], k[±2]·k[±2], k[0]·k[0]
ZERO, ONE = _v(0, 0, 0), _v(1, 1, 1)


def base(L, k, axis="row"):
    """n_A = (0,0,1), n_B = (0,0,1/2), P_A = 0, P_B = (1,0,1), sigma_plane = 1, e_A = 0, e_B = (1,1,1), sigma_color = 2^(L-1).
    wn = (1/2)^(2^k) both ways.  v = ±(1,0,1), d2 = 2.  From A: pl = 1, u = 1 - 1/2, wz = 1/4.  From B: pl = -1/2 (B's OWN normal),
    u = 1 - (1/4)/2 = 7/8, wz = 49/64.  dot(de,de)·4^(L-1) / 4^(L-1) = 3, wc = 1/4.  A's centre: g = 1; B's: g = (1/4)^(2^k), wz = wc = 1.
    out_A = w / (9/64 + w), w = h·wn·(1/4)·(1/4);  out_B = c / (c + w'), c = 9/64·(1/4)^(2^k), w' = h·wn·(49/64)·(1/4)."""
    h = HD if axis == "diag" else H2
    wn = F(1, 2) ** (2 ** k)
    w = h * wn * F(1, 4) * F(1, 4)
    c = C0 * F(1, 4) ** (2 ** k)
    w2 = h * wn * F(49, 64) * F(1, 4)
    return pair(f"base-{axis}-L{L}-k{k}", base.__doc__, L, k, mix(C0, ZERO, w, ONE), mix(c, ONE, w2, ZERO), axis=axis)


def cases():
    out = [base(L, k) for L in range(1, 9) for k in (0, 1, 3)]
    # the column form (tap j = ±2, h = k[0]·k[2] = 3/128 as well) and a diagonal pair (i = j = ±2: h = 1/256)
    out += [base(2, 1, "col"), base(5, 0, "col"), base(3, 1, "diag"), base(1, 3, "diag")]

    # normal_power_log2 = 16.  n_B = (0.6f, 0, 0.8f): n_A.n_B = 0.8f and 0.8^65536 < 2^-21000 is 0 in f32 long before the 16th
    # squaring, so each pixel adds fma(0, e_other, S) = S and + 0 to W: S / W = (c·e) / c with c = 9/64·g_c > 0.  g_c is NOT a
    # rational of this file: n_B.n_B = 1 + d with |d| < 2^-22 in f32 (three roundings of values <= 1), so g_c = (1 + d)^65536 lies
    # in (0.98, 1.02), positive and finite — and that is all that matters: e_B's channels are powers of two, so c·e_B is exact
    # and S / W = e_B for ANY such c; e_A has 2 significant bits and A's c is 9/64 exactly (n_A.n_A = 1).
    eA, eB = _v(F(3, 4), F(1, 2), F(1, 4)), _v(1, F(1, 2), 2)
    out.append(pair("npl16-underflow", "wn = 0.8^65536 underflows to 0: each pixel keeps its centre value exactly", 2, 16, list(eA), list(eB),
                    n_b=(float(np.float32(0.6)), 0, float(np.float32(0.8))), c_a=eA, c_b=eB, general=False))

    # dot(n_A, n_B) = -1/2 < 0: max0 gives wn = 0 for EVERY power (without max0 an even power would give (1/2)^(2^k) > 0), w = 0,
    # both pixels keep their centre value: S / W = (c·e) / c = e.  (e_A ≠ 0 here, so a leak from either side shows.)
    for k in (0, 1, 3):
        out.append(pair(f"backfacing-k{k}", "n_A.n_B = -1/2: max0 makes wn = 0 before any squaring, centre values stay", 3, k, list(eA), list(eB),
                        n_b=(0, 0, F(-1, 2)), c_a=eA, c_b=eB))

    # d2 == 0 with different normals: P_A = P_B, so wz = 1 from both sides whatever the normals are; wn = (1/2)^(2^k), wc = 1/4.
    # out_A = w / (9/64 + w), out_B = c / (c + w), w = 3/128·wn·1·(1/4), c = 9/64·(1/4)^(2^k).
    for k in (0, 2):
        wn, c = F(1, 2) ** (2 ** k), C0 * F(1, 4) ** (2 ** k)
        w = H2 * wn * F(1, 4)
        out.append(pair(f"same-point-k{k}", "d2 = 0: wz = 1 for any normals", 4, k, mix(C0, ZERO, w, ONE), mix(c, ONE, w, ZERO), P_b=(0, 0, 0)))

    # u clamps to 0.  AT sigma_plane: P_B = (0,0,1), sigma_plane = 1: from A pl = 1, d2 = 1, u = max0(1 - 1/1) = 0, wz = 0, out_A = e_A.
    # From B (k = 0): pl = -1/2, u = 1 - 1/4 = 3/4, wz = 9/16 — NOT clamped: out_B = c / (c + w'), c = 9/64·1/4, w' = 3/128·(1/2)·(9/16)·(1/4).
    w2 = H2 * F(1, 2) * F(9, 16) * F(1, 4)
    out.append(pair("plane-at-sigma", "pl^2 = sp2·d2 from A: u = 0 exactly; from B u = 3/4", 2, 0, list(ZERO), mix(C0 / 4, ONE, w2, ZERO), P_b=(0, 0, 1)))
    # BEYOND: P_B = (1,0,1), sigma_plane = 1/2: from A pl = 1, ratio = 1 / (1/4·2) = 2, u = max0(-1) = 0 (unclamped, u·u would be 1).
    # From B: pl = -1/2, ratio = (1/4) / (1/2) = 1/2, wz = 1/4: out_B = c / (c + w'), w' = 3/128·(1/2)·(1/4)·(1/4).
    w2 = H2 * F(1, 2) * F(1, 4) * F(1, 4)
    out.append(pair("plane-beyond-sigma", "pl^2 = 2·sp2·d2 from A: u = max0(-1) = 0; from B wz = 1/4", 3, 0, list(ZERO), mix(C0 / 4, ONE, w2, ZERO),
                    sigma_plane=F(1, 2)))

    # demodulation.  a_A = (1/2, 1, 2^-10), a_B = (1/4, 2^-10, 1/2): m = max(a, 2^-8) = (1/2, 1, 2^-8) and (1/4, 2^-8, 1/2).  c_A = 0,
    # c_B = m_B, so e_A = 0, e_B = (1,1,1): de = (1,1,1) although dc = m_B — the colour distance on c would give wc = 1 / (1 + 5/16 + 2^-16).
    # The filter is the base case's (k = 1): out = base·m per channel, m a power of two, so the product is exact.  Without the floor
    # e_B,g = 2^-8 / 2^-10 = 4.
    wn = F(1, 4)
    w, c, w2 = H2 * wn * F(1, 4) * F(1, 4), C0 * F(1, 16), H2 * wn * F(49, 64) * F(1, 4)
    mB = _v(F(1, 4), F(1, 256), F(1, 2))
    out.append(pair("demodulated", "e = c / max(a, 2^-8) is (0,0,0) and (1,1,1): the base case on e, times m", 3, 1, mix(C0, ZERO, w, ONE),
                    mix(c, ONE, w2, ZERO), c_b=mB, a_a=_v(F(1, 2), 1, F(1, 1024)), a_b=_v(F(1, 4), F(1, 1024), F(1, 2))))

    # a stride-1 pair: 1 row x 2 columns, one level, the i = ±1 tap: h = k[1]·k[0] = 3/32, 4^0 = 1, sigma_color = 1: the base case's
    # weights with h = 3/32 (k = 1).
    w, w2 = H1 * wn * F(1, 4) * F(1, 4), H1 * wn * F(49, 64) * F(1, 4)
    out.append(pair("stride1-2x1", "the i = ±1 tap, h = 3/32", 1, 1, mix(C0, ZERO, w, ONE), mix(c, ONE, w2, ZERO), span=1, sigma_color=1.0))
    out.append(nine())
    out.append(zero_normal())
    return out


def nine():
    """3x3, all hits, one level, normal_power_log2 = 0, sigma_plane = sigma_color = 1.  n = (0,0,z) with z a power of two, so
    wn = z_p·z_q; P in {0, (1,0,0), (0,0,1), (1,0,1)}: d2 in {0, 1, 2}, pl = z_p·dz, u = 1 - z_p^2·dz^2 / d2; e in {(0,0,0), (1,1,1)}:
    wc in {1, 1/4}.  The nine weights of the centre pixel are pairwise different (asserted by the CPU test); every one of the 81 is
    a dyadic of few bits and S, W are exact sums, so each output is one rounded divide.  No closed form is written out for 81
    weights: exact() is the statement, and it is pinned by every other case's `hand`."""
    z = np.array([[0.5, 0.125, 0.25], [0.25, 0.25, 0.5], [0.5, 0.25, 0.5]], np.float32)
    pts = {0: (0, 0, 0), 1: (1, 0, 0), 2: (0, 0, 1), 3: (1, 0, 1)}
    which = np.array([[3, 3, 1], [2, 0, 2], [0, 0, 0]])
    col = np.array([[0, 1, 0], [1, 0, 1], [1, 0, 0]], np.float32)
    index = np.arange(9, dtype=np.int32).reshape(3, 3)
    normal = np.zeros((3, 3, 3), np.float32)
    normal[..., 2] = z
    point = np.array([[pts[k] for k in row] for row in which], np.float32)
    rgb = np.repeat(col[..., None], 3, axis=2)
    case = Case("nine-weights-3x3", nine.__doc__, rgb, index, normal, point, None,
                dict(levels=1, normal_power_log2=0, flags=0, sigma_color=1.0, sigma_plane=1.0), None)
    case.hand = exact(case)
    return case


def zero_normal():
    """What §4.11 does NOT promise: 5x5 hits on one plane (n = (0,0,1), P = (x, y, 0): wn = wz = 1), sigma_color = +inf (wc = 1), one
    level — and the centre pixel Z = (2,2) has the normal (0,0,0) of a degenerate guide.  At Z every wn is 0: W = 0, S = 0, the output
    is 0/0 = NaN.  For every other pixel p the tap on Z has the honest weight 0 with a finite e_Z = 64: it adds 0 to W and leaves S.
    With A(0) = A(4) = 11/16, A(1) = A(3) = 15/16, A(2) = 1 the sums of k over the taps in the frame, W_p = A(x)·A(y) - k[2-x]·k[2-y],
    and the image is an impulse of 1 at I = (0,1) (row 0, column 1) besides Z: out_p = k[1-x]·k[0-y] / W_p where I is a tap of p, else 0."""
    index = np.arange(25, dtype=np.int32).reshape(5, 5)
    normal = np.zeros((5, 5, 3), np.float32)
    normal[..., 2] = 1
    normal[2, 2] = 0
    point = np.zeros((5, 5, 3), np.float32)
    point[..., 0], point[..., 1] = np.meshgrid(np.arange(5), np.arange(5))
    rgb = np.zeros((5, 5, 3), np.float32)
    rgb[2, 2] = 64
    rgb[0, 1] = 1
    A = {0: F(11, 16), 1: F(15, 16), 2: F(1), 3: F(15, 16), 4: F(11, 16)}
    hand = {}
    for y in range(5):
        for x in range(5):
            if (y, x) == (2, 2):
                hand[(y, x)] = None
                continue
            W = A[x] * A[y] - K[2 - x] * K[2 - y]
            i, j = 1 - x, 0 - y
            hand[(y, x)] = [K[i] * K[j] / W if abs(i) <= 2 and abs(j) <= 2 else F(0)] * 3
    return Case("zero-normal-5x5", zero_normal.__doc__, rgb, index, normal, point, None,
                dict(levels=1, normal_power_log2=6, flags=0, sigma_color=INF, sigma_plane=0.25), hand)
