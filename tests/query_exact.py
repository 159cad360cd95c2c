"""An exact `findHit` for the query tests, independent of the library: rational arithmetic (fractions.Fraction) on the exact
values a query kernel receives — the scene's own f64 values, the rays as given (f32 rays are their f32 values), tmin as the
kernel holds it (rounded to the precision) — with decimal square roots at 80 digits where a sphere root is irrational.  No float
decides anything: floats only bound errors and pick candidate pairs.

Per ray, `exact_find_hit` gives every exact root in [tmin, tmax] with its hittable (spheres first, then triangles), sorted; the
winner (nearest, ties to the larger index), its exact point, outward normal ((p - centre) / r for a
sphere, the direction of cross(v1 - v0, v2 - v0) for a triangle), front_face, material and albedo (the checker chain walked
with exact floor parity); and how near each decision came to flipping.

Error bounds (u = 2^-24 for F32, 2^-53 for F64; u64 = 2^-53; every bound below is the first-order sum of the roundings named,
doubled to cover the higher-order terms):
- Sphere (both precisions decide in f64 on the pool's f64 sphere, §4.3): with q = c + v·time - o, a = d·d, M = |q|² + r² + |q||v|,
  q carries 2 u64 (|q| + |v|) (c - o, then the FMA), hb = d·q 3 u64 |d||q| + |d| Δq, cc = q·q - r² 4 u64 M + 2 |q| Δq, so
  ΔD = 2 · 16 u64 · a · M for D = hb² - a·cc.  A root t = (hb ± √D) / a then carries
  Δt = 2 [(5 u64 |d| (|q| + |v|) + min(√ΔD, ΔD / √D) + u64 (|hb| + √D)) / a + 6 u64 |t|] + (F32) u |t| (the root rounded to f32).
  |D| ≤ ΔD is a maybe-root near hb / a with Δt = 2 √(2 ΔD) / a plus the above.
- Triangle (Möller–Trumbore in R on R(v0), e1 = R(v1 - v0), e2 = R(v2 - v0)): with S = o - v0, E1, E2 exact
  and |S| standing for |o - v0| + |v0| (the kernel's sv = R(o - R(v0)) carries u (|o - v0| + |v0|)), the kernel's det = e1·(d × e2), A1 = sv·(d × e2), A2 = d·(sv × e1) are within Δdet = 2·7u |E1||d||E2|,
  ΔA1 = 2·7u |S||d||E2|, ΔA2 = 2·7u |S||d||E1| (one rounding for each of e, sv, two for a cross, three for a dot); its filter
  (A1·det ≥ 0, A2·det ≥ 0, det·(det - A1 - A2) ≥ 0, each product rounded once more: + 4u (|A1| + |A2| + |det|)) surely passes
  when the whole error box passes and surely fails when none of it can; t = (e2·(sv × e1)) / det carries
  Δt = 2u (8 |S||E1||E2| + (7 |E1||d||E2| + |det|) |t|) / (|det| - Δdet), unbounded when |det| ≤ Δdet.
- Point o + t·d (one FMA in R): Δp = |d| Δt + 2u (|o| + |d||t|) per component.  Sphere normal unit(p - c(time)):
  Δn = 2 (Δp + 3u (|c| + |v|) + u |p|) / r + 6u (c, v rounded to R).  Triangle normal unit(cross(e1, e2)):
  Δn = 8u |E1||E2| / |E1 × E2| + 6u.  front_face = n·d < 0 is decided when |n·d| / |d| > 2 (Δn + 3u).  Checker parity
  floor(p_k / scale): decided when p_k / scale lies farther than 2 (Δp / scale + 3u |p_k / scale|) from an integer.

A candidate pair is a (ray, hittable) pair the kernel COULD accept: `_candidates` evaluates D (spheres) and det, A1, A2
(triangles) in float64 for every pair and keeps a pair unless even twice the bound above rules it out.  float64 evaluation
carries at most the same bound with u64 ≤ u, so the kept set is a proven superset; the exact work stays proportional to the
hits, as in tests/query_reference._pairs_near."""
import math
from decimal import Decimal, getcontext
from fractions import Fraction as Fr

import numpy as np

from rayz_amd import capi

getcontext().prec = 80
U64 = 2.0 ** -53
INF = float("inf")


def u_of(precision):
    return 2.0 ** -24 if precision == capi.PRECISION_F32 else U64


def _dec(x: Fr) -> Decimal:
    return Decimal(x.numerator) / Decimal(x.denominator)


def _sqrt_fr(x: Fr):
    """√x as a Fraction when x is a rational square, else None."""
    n, d = x.numerator, x.denominator
    a, b = math.isqrt(n), math.isqrt(d)
    return Fr(a, b) if a * a == n and b * b == d else None


class Root:
    """P + s·√Q exactly (Q ≥ 0 rational; Q = 0 when the root is rational), with an 80-digit value."""
    __slots__ = ("P", "s", "Q", "val")

    def __init__(self, P: Fr, s: int, Q: Fr):
        r = _sqrt_fr(Q)
        if r is not None:
            P, s, Q = P + s * r, 0, Fr(0)
        self.P, self.s, self.Q = P, s, Q
        self.val = _dec(P) + (s * _dec(Q).sqrt() if s else Decimal(0))

    def ge(self, x: Fr) -> bool:  # exactly: self >= x
        if self.s == 0:
            return self.P >= x
        y = x - self.P
        return (y <= 0 or self.Q >= y * y) if self.s > 0 else (y <= 0 and y * y >= self.Q)

    def le(self, x: Fr) -> bool:  # exactly: self <= x
        if self.s == 0:
            return self.P <= x
        y = x - self.P
        return (y >= 0 and y * y >= self.Q) if self.s > 0 else (y >= 0 or self.Q >= y * y)

    def same(self, o: "Root") -> bool:  # exact equality (irrational parts are equal only with equal P, s, Q)
        return self.P == o.P and self.s == o.s and self.Q == o.Q


def _v(a):
    return [Fr(float(x)) for x in a]


def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _norm(a):
    return math.sqrt(sum(float(x) * float(x) for x in a))


class Scene:
    """The pool of a SceneDesc: float64 arrays for the candidate search, Fractions for the exact work."""

    def __init__(self, sd: capi.SceneDesc):
        ns, nt = sd.n_spheres, sd.n_triangles
        self.sd, self.ns, self.nt = sd, ns, nt
        self.c = np.array([list(sd.spheres[i].center) for i in range(ns)], np.float64).reshape(-1, 3)
        self.v = np.array([list(sd.spheres[i].velocity) for i in range(ns)], np.float64).reshape(-1, 3)
        self.r = np.array([sd.spheres[i].radius for i in range(ns)], np.float64)
        self.tri = np.array([[list(sd.triangles[i].v0), list(sd.triangles[i].v1), list(sd.triangles[i].v2)] for i in range(nt)],
                            np.float64).reshape(-1, 3, 3)
        self.mat = np.array([sd.spheres[i].material for i in range(ns)] + [sd.triangles[i].material for i in range(nt)], np.int64)


def _candidates(S: Scene, rays, u):
    """(ray, hittable) pairs that the kernel could accept, by float64 evaluation with twice the error bound (module docstring)."""
    pr, pi = [], []
    o, d, tm = rays[:, 0:3], rays[:, 4:7], rays[:, 3]
    with np.errstate(all="ignore"):
        for a0 in range(0, len(rays), 256):
            sl = slice(a0, a0 + 256)
            if S.ns:
                q = S.c[None] + S.v[None] * tm[sl, None, None] - o[sl, None, :]
                dd = d[sl, None, :]
                a = (dd * dd).sum(-1)
                hb = (dd * q).sum(-1)
                qq = (q * q).sum(-1)
                M = qq + S.r[None] ** 2 + np.sqrt(qq) * np.linalg.norm(S.v, axis=1)[None]
                D = hb * hb - a * (qq - S.r[None] ** 2)
                keep = D >= -2 * 32 * U64 * a * M * 2
                ri, ci = np.nonzero(keep)
                pr.append(ri + a0), pi.append(ci)
            if S.nt:
                v0, E1, E2 = S.tri[:, 0], S.tri[:, 1] - S.tri[:, 0], S.tri[:, 2] - S.tri[:, 0]
                Sv = o[sl, None, :] - v0[None]
                dd = np.broadcast_to(d[sl, None, :], Sv.shape)
                P = np.cross(dd, E2[None])
                det = (E1[None] * P).sum(-1)
                A1 = (Sv * P).sum(-1)
                A2 = (dd * np.cross(Sv, E1[None])).sum(-1)
                nd, nS = np.linalg.norm(dd, axis=-1), np.linalg.norm(Sv, axis=-1) + np.linalg.norm(v0, axis=1)[None]
                n1, n2 = np.linalg.norm(E1, axis=1)[None], np.linalg.norm(E2, axis=1)[None]
                k = 2 * 2 * 7 * u  # twice the kernel's bound, which also covers the float64 evaluation's own
                ed, e1, e2 = k * n1 * nd * n2, k * nS * nd * n2, k * nS * nd * n1
                ew = ed + e1 + e2 + 8 * u * (np.abs(A1) + np.abs(A2) + np.abs(det))
                pos = (det + ed > 0) & (A1 + e1 >= 0) & (A2 + e2 >= 0) & \
                      (np.maximum(A1 - e1, 0) + np.maximum(A2 - e2, 0) <= det + ed + ew)
                neg = (det - ed < 0) & (A1 - e1 <= 0) & (A2 - e2 <= 0) & \
                      (np.minimum(A1 + e1, 0) + np.minimum(A2 + e2, 0) >= det - ed - ew)
                keep = pos | neg | ~np.isfinite(det)
                ri, ci = np.nonzero(keep)
                pr.append(ri + a0), pi.append(ci + S.ns)
    if not pr:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(pr), np.concatenate(pi)


class Hit:
    """One way the kernel may answer a ray: hittable `index` at exact `t` (a Root; None: any t) within `dt`; `sure` when the kernel
    must take it (no error bound reaches a decision)."""
    __slots__ = ("index", "t", "dt", "sure", "info")

    def __init__(self, index, t, dt, sure, info):
        self.index, self.t, self.dt, self.sure, self.info = index, t, dt, sure, info

    def lo(self):
        return -INF if self.t is None else float(self.t.val) - self.dt

    def hi(self):
        return INF if self.t is None else float(self.t.val) + self.dt


def _sphere(S, k, o, d, time, tmin, tmax, u, f32):
    """(exact roots in [tmin, tmax], the options the kernel may take for this sphere, the discriminant margin)."""
    c, v, r = _v(S.c[k]), _v(S.v[k]), Fr(float(S.r[k]))
    q = [c[i] + v[i] * time - o[i] for i in range(3)]
    a, hb, cc = _dot(d, d), _dot(d, q), _dot(q, q) - r * r
    D = hb * hb - a * cc
    fa, fq, fv, fhb = float(a), _norm(q), _norm(v), float(hb)
    M = fq * fq + float(r) ** 2 + fq * fv
    dD = 2 * 16 * U64 * fa * M
    roots = []
    if D >= 0:
        P, Q = hb / a, D / (a * a)
        roots = [Root(P, -1, Q), Root(P, 1, Q)] if Q else [Root(P, 0, Q)]
    inrange = [x for x in roots if x.ge(tmin) and (tmax is None or x.le(tmax))]
    fD = float(D)
    sq = math.sqrt(max(fD, 0.0))

    def dt_of(t):
        dsq = min(math.sqrt(dD), dD / sq) if sq > 0 else math.sqrt(dD)
        e = 2 * ((5 * U64 * math.sqrt(fa) * (fq + fv) + dsq + U64 * (abs(fhb) + sq)) / fa + 6 * U64 * abs(t))
        return e + (u * abs(t) if f32 else 0.0)

    opts = []
    if abs(fD) <= dD:  # a maybe-root near the double root
        t0 = Root(hb / a, 0, Fr(0))
        opts.append(Hit(k, t0, dt_of(float(t0.val)) + 2 * math.sqrt(2 * dD) / fa, False, ("sphere", k)))
        return inrange, opts, fD / max(fa * M, 1e-300)
    if D < 0:
        return inrange, opts, fD / (fa * M)
    # the kernel takes the near root if it rounds to >= tmin, else the far one; either may be cut by tmax
    ftmin, ftmax = float(tmin), (INF if tmax is None else float(tmax))
    for x in roots:
        t = float(x.val)
        e = dt_of(t)
        below = t + e < ftmin
        if below:
            continue
        sure_in = t - e > ftmin and t + e < ftmax
        if t - e <= ftmax:
            opts.append(Hit(k, x, e, sure_in, ("sphere", k)))
        if t - e > ftmin:  # this root surely is the one the kernel takes (>= tmin); the far one is never reached
            break
    return inrange, opts, fD / (fa * M)


def _triangle(S, j, o, d, tmin, tmax, u):
    k = j - S.ns
    v0, v1, v2 = _v(S.tri[k, 0]), _v(S.tri[k, 1]), _v(S.tri[k, 2])
    E1, E2, Sv = _sub(v1, v0), _sub(v2, v0), _sub(o, v0)
    Pv, Qv = _cross(d, E2), _cross(Sv, E1)
    det, A1, A2 = _dot(E1, Pv), _dot(Sv, Pv), _dot(d, Qv)
    n1, n2, nS, nd = _norm(E1), _norm(E2), _norm(Sv) + _norm(v0), _norm(d)
    ed, e1, e2 = 2 * 7 * u * n1 * nd * n2, 2 * 7 * u * nS * nd * n2, 2 * 7 * u * nS * nd * n1
    fdet, fA1, fA2 = float(det), float(A1), float(A2)
    ew = ed + e1 + e2 + 4 * u * (abs(fA1) + abs(fA2) + abs(fdet))
    inrange, t = [], None
    bary = -INF
    if det != 0:
        b1, b2 = A1 / det, A2 / det
        mb = min(b1, b2, 1 - b1 - b2)
        bary = float(mb)
        t = Root(_dot(E2, Qv) / det, 0, Fr(0))
        if mb >= 0 and t.ge(tmin) and (tmax is None or t.le(tmax)):
            inrange = [t]
    sgn = 1 if fdet >= 0 else -1
    sure_pass = abs(fdet) > ed and sgn * fA1 > e1 and sgn * fA2 > e2 and sgn * (fA1 + fA2) + e1 + e2 + ew < abs(fdet) - ed
    may_pos = (fdet + ed > 0) and fA1 + e1 >= 0 and fA2 + e2 >= 0 and max(fA1 - e1, 0) + max(fA2 - e2, 0) <= fdet + ed + ew
    may_neg = (fdet - ed < 0) and fA1 - e1 <= 0 and fA2 - e2 <= 0 and min(fA1 + e1, 0) + min(fA2 + e2, 0) >= fdet - ed - ew
    opts = []
    if sure_pass or may_pos or may_neg:
        if abs(fdet) > ed and t is not None:
            ft = float(t.val)
            e = 2 * u * (8 * nS * n1 * n2 + (7 * n1 * nd * n2 + abs(fdet)) * abs(ft)) / (abs(fdet) - ed)
            if ft + e >= float(tmin) and (tmax is None or ft - e <= float(tmax)):
                sure = sure_pass and ft - e > float(tmin) and (tmax is None or ft + e < float(tmax))
                opts.append(Hit(j, t, e, sure, ("triangle", k)))
        else:
            opts.append(Hit(j, None, INF, False, ("triangle", k)))
    return inrange, opts, bary


def _tex_albedo(sd, material, p_dec, dp, u, precision):
    """(albedo, decided): the texture chain walked at the exact point with exact floor parity; decided = every cell decision's
    margin exceeds its bound.  Also the smallest cell-boundary distance (in cells)."""
    m = sd.materials[material]
    if m.kind == capi.MAT_DIELECTRIC:
        return np.ones(3), True, INF
    idx, margin, ok = m.texture, INF, True
    for _ in range(8):
        t = sd.textures[idx]
        if t.kind == capi.TEX_SOLID:
            col = np.array(list(t.color))
            return (col.astype(np.float32).astype(np.float64) if precision == capi.PRECISION_F32 else col), ok, margin
        sc = Decimal(float(t.scale))
        s = 0
        for kk in range(3):
            x = p_dec[kk] / sc
            fx = x.to_integral_value(rounding="ROUND_FLOOR")
            s += int(fx)
            dist = float(min(x - fx, fx + 1 - x))
            margin = min(margin, dist)
            if dist <= 2 * (dp / float(t.scale) + 3 * u * abs(float(x))):
                ok = False
        idx = t.even if s % 2 == 0 else t.odd
    return np.zeros(3), ok, margin


class ExactRay:
    """The exact answer for one ray (see the module docstring) and the options the kernel may take."""
    __slots__ = ("roots", "winner", "options", "miss_ok", "disc_margin", "bary_margin", "gap", "range_margin", "point", "normal",
                 "front_face", "material", "albedo", "checker_margin")


def _record(S: Scene, e: ExactRay, o, d, R, precision):
    """The winner's exact record: point o + t·d and outward normal (80 digits, then float64), front_face decided exactly (a
    sphere's (p - c)·d = a·(t - hb/a) is negative at the near root, a triangle's cross(E1, E2)·d is rational), material, albedo."""
    t, j = e.winner
    p_dec = [_dec(o[k]) + _dec(d[k]) * t.val for k in range(3)]
    e.point = np.array([float(x) for x in p_dec])
    if j < S.ns:
        time = Fr(float(R[3]))
        cd = [_dec(Fr(float(S.c[j, k])) + Fr(float(S.v[j, k])) * time) for k in range(3)]
        r = Decimal(abs(float(S.r[j])))  # (the reference normalises p - c: a negative radius is its magnitude)
        e.normal = np.array([float((p_dec[k] - cd[k]) / r) for k in range(3)])
        q = [Fr(float(S.c[j, k])) + Fr(float(S.v[j, k])) * time - o[k] for k in range(3)]
        e.front_face = not t.ge(_dot(d, q) / _dot(d, d))  # t < hb / a: the near root
    else:
        k = j - S.ns
        cr = _cross(_sub(_v(S.tri[k, 1]), _v(S.tri[k, 0])), _sub(_v(S.tri[k, 2]), _v(S.tri[k, 0])))
        ln = sum(_dec(x) ** 2 for x in cr).sqrt()
        e.normal = np.array([float(_dec(x) / ln) for x in cr])
        e.front_face = _dot(cr, d) < 0
    e.material = int(S.mat[j])
    e.albedo, _, e.checker_margin = _tex_albedo(S.sd, e.material, p_dec, 0.0, 0.0, precision)


def exact_find_hit(sd: capi.SceneDesc, rays, tmin: float, precision: int, scene: Scene = None):
    """A list of ExactRay, one per ray of `rays` ((n, 8) float64 holding values of the precision).  `tmin` is rounded to the
    precision as the kernel holds it."""
    S = scene or Scene(sd)
    f32 = precision == capi.PRECISION_F32
    u = u_of(precision)
    rays = np.asarray(rays, np.float64)
    tmin_r = float(np.float32(tmin)) if f32 else float(tmin)
    ftmin = Fr(tmin_r)
    ri, pi = _candidates(S, rays, u)
    order = np.lexsort((pi, ri))
    ri, pi = ri[order], pi[order]
    starts = np.searchsorted(ri, np.arange(len(rays) + 1))
    out = []
    for n in range(len(rays)):
        R = rays[n]
        o, d, time = _v(R[0:3]), _v(R[4:7]), Fr(float(R[3]))
        tmax = None if R[7] == INF else Fr(float(R[7]))
        e = ExactRay()
        e.roots, e.options, e.disc_margin, e.bary_margin = [], [], INF, INF
        for j in pi[starts[n]:starts[n + 1]]:
            j = int(j)
            if j < S.ns:
                inr, opts, m = _sphere(S, j, o, d, time, ftmin, tmax, u, f32)
                e.disc_margin = min(e.disc_margin, abs(m))
            else:
                inr, opts, m = _triangle(S, j, o, d, ftmin, tmax, u)
                e.bary_margin = min(e.bary_margin, abs(m))
            e.roots += [(x, j) for x in inr]
            e.options += opts
        e.roots.sort(key=lambda xj: (xj[0].val, -xj[1]))
        # the exact winner: the nearest root, ties (exactly equal roots) to the larger index
        e.winner = None
        if e.roots:
            best = e.roots[0]
            for x, j in e.roots[1:]:
                if x.same(best[0]) and j > best[1]:
                    best = (x, j)
            e.winner = best
        # the options that can be the kernel's minimum: every option whose window starts before the nearest SURE option ends
        sure_hi = min([h.hi() for h in e.options if h.sure], default=INF)
        e.options = [h for h in e.options if h.lo() <= sure_hi]
        e.miss_ok = not any(h.sure for h in e.options)
        e.gap = INF
        e.range_margin = INF
        e.point = e.normal = e.albedo = None
        e.front_face, e.material, e.checker_margin = False, -1, INF
        if e.winner is not None:
            _record(S, e, o, d, R, precision)
            tw = e.winner[0].val
            others = [x.val for x, j in e.roots if j != e.winner[1]]
            e.gap = float(min([abs(x - tw) for x in others], default=Decimal("Infinity")))
            e.range_margin = float(min(tw - _dec(ftmin), (_dec(tmax) - tw) if tmax is not None else Decimal("Infinity")))
        out.append(e)
    return out


def unambiguous(e: ExactRay) -> bool:
    """One answer only: a sure winner alone among the options, or a sure miss."""
    if e.winner is None:
        return not e.options
    return len(e.options) >= 1 and all(h.index == e.winner[1] for h in e.options) and not e.miss_ok


def check_exact(sd: capi.SceneDesc, rays, got: dict, exact, precision: int, scene: Scene = None):
    """Asserts the kernel's answers `got` (query outputs as numpy arrays) against `exact` (exact_find_hit) within the bounds of
    the module docstring; returns a summary: the unambiguous fraction and the largest error / bound ratios."""
    S = scene or Scene(sd)
    f32 = precision == capi.PRECISION_F32
    u = u_of(precision)
    rays = np.asarray(rays, np.float64)
    idx = got["index"].astype(np.int64)
    n_unamb, worst = 0, {"t": 0.0, "point": 0.0, "normal": 0.0}
    n_albedo = 0
    for n, e in enumerate(exact):
        i = int(idx[n])
        if unambiguous(e):
            n_unamb += 1
            want = e.winner[1] if e.winner is not None else -1
            assert i == want, f"ray {n}: index {i}, the exact winner is {want} (unambiguous)"
        if i < 0:
            assert e.miss_ok, f"ray {n}: a miss, but a hit is certain ({[h.index for h in e.options]})"
            assert got["material"][n] == -1 and np.isinf(got["t"][n]), n
            for k in ("point", "normal", "front_face", "albedo"):
                assert k not in got or (got[k][n] == 0).all(), (n, k, got[k][n])
            continue
        opts = [h for h in e.options if h.index == i]
        assert opts, f"ray {n}: index {i} is not among the possible answers {[h.index for h in e.options]} (winner {e.winner and e.winner[1]})"
        assert got["material"][n] == S.mat[i], (n, got["material"][n], S.mat[i])  # always exact
        tg = float(got["t"][n])
        h = min(opts, key=lambda h: 0.0 if h.t is None else abs(float(h.t.val) - tg))
        if h.t is None:
            continue  # a degenerate triangle test: the index is possible, no value is pinned
        ferr = abs(float(h.t.val) - tg)
        assert ferr <= h.dt, f"ray {n}: t {tg!r}, exact {float(h.t.val)!r}, bound {h.dt:.3g}"
        worst["t"] = max(worst["t"], ferr / h.dt if h.dt else 0.0)
        if "point" not in got or not got.get("record", np.ones(len(rays), bool))[n]:
            continue  # (mode B has no triangle record: index, t and material only)
        o, d = rays[n, 0:3], rays[n, 4:7]
        nd, no = float(np.abs(d).max()), float(np.abs(o).max())
        tv = h.t.val
        p_dec = [Decimal(float(o[k])) + Decimal(float(d[k])) * tv for k in range(3)]
        p_ex = np.array([float(x) for x in p_dec])
        dp = nd * h.dt + 2 * u * (no + nd * abs(float(tv)))
        perr = float(np.abs(got["point"][n] - p_ex).max())
        assert perr <= dp, f"ray {n}: point {got['point'][n]}, exact {p_ex}, bound {dp:.3g}"
        worst["point"] = max(worst["point"], perr / dp)
        if i < S.ns:
            cd = [Decimal(float(S.c[i, k])) + Decimal(float(S.v[i, k])) * Decimal(float(rays[n, 3])) for k in range(3)]
            r = abs(float(S.r[i]))
            nrm = np.array([float((p_dec[k] - cd[k]) / Decimal(r)) for k in range(3)])
            dn = 2 * (dp + 3 * u * (float(np.abs(S.c[i]).max()) + float(np.abs(S.v[i]).max())) + u * float(np.abs(p_ex).max())) / r + 6 * u
        else:
            k = i - S.ns
            E1, E2 = _sub(_v(S.tri[k, 1]), _v(S.tri[k, 0])), _sub(_v(S.tri[k, 2]), _v(S.tri[k, 0]))
            cr = [_dec(x) for x in _cross(E1, E2)]
            ln = (cr[0] ** 2 + cr[1] ** 2 + cr[2] ** 2).sqrt()
            nrm = np.array([float(x / ln) for x in cr])
            dn = 8 * u * _norm(E1) * _norm(E2) / float(ln) + 6 * u
        # front_face: n·d < 0, decided where the margin exceeds the bound; the stored normal faces the ray
        cosv = float(sum(Decimal(float(nrm[k])) * Decimal(float(d[k])) for k in range(3))) / float(np.linalg.norm(d))
        ff = int(got["front_face"][n])
        if abs(cosv) > 2 * (dn + 3 * u):
            assert ff == (1 if cosv < 0 else 0), f"ray {n}: front_face {ff}, n·d/|d| = {cosv:.3g} (bound {2 * (dn + 3 * u):.3g})"
        want_n = nrm if ff == 1 else -nrm
        nerr = float(np.abs(got["normal"][n] - want_n).max())
        assert nerr <= dn, f"ray {n}: normal {got['normal'][n]}, exact {want_n}, bound {dn:.3g}"
        worst["normal"] = max(worst["normal"], nerr / dn)
        if "albedo" in got:
            alb, ok, _ = _tex_albedo(sd, int(S.mat[i]), p_dec, dp, u, precision)
            if ok:
                n_albedo += 1
                assert np.array_equal(got["albedo"][n].astype(np.float64), alb), (n, got["albedo"][n], alb)
    return {"rays": len(exact), "unambiguous": n_unamb / max(1, len(exact)), "albedo_decided": n_albedo,
            "worst_over_bound": worst}
