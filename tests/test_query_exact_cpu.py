"""The exact `findHit` reference (tests/query_exact.py) without a GPU: held to hand-derived answers, then used to hold the mode-B
brute force (the restatement the query kernels match bit for bit) to the error bounds of its docstring on every query scene; and
the direction-scale covariance of the mode-B pieces over the accepted direction range (include/rayz_hip.h,
RAYZ_QUERY_MIN_DIR / RAYZ_QUERY_MAX_DIR), with a factor 2^16 to spare on either side."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from query_exact import Scene, check_exact, exact_find_hit, unambiguous
from query_reference import SCENES, TMIN, brute_force, ray_mix
from rayz_amd import capi
from test_query_cpu import _pool, _ray

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _one(sd, ray, tmin=1e-3, precision=F64):
    return exact_find_hit(sd, np.array([ray]), tmin, precision)[0]


def test_exact_reference_on_hand_built_cases():
    still = (0.0, 0.0, 0.0)
    s0 = ((0.0, 0.0, -5.0), 1.0, still)  # unit sphere at z = -5 seen from the origin along -z: roots exactly 4 and 6
    sd = _pool([s0])
    e = _one(sd, _ray((0, 0, 0), (0, 0, -1)))
    assert [(float(x.val), j) for x, j in e.roots] == [(4.0, 0), (6.0, 0)]
    assert e.winner[1] == 0 and float(e.winner[0].val) == 4.0 and unambiguous(e)
    assert e.point.tolist() == [0.0, 0.0, -4.0] and e.normal.tolist() == [0.0, 0.0, 1.0] and e.front_face and e.material == 0
    assert e.gap == np.inf and e.range_margin == pytest.approx(4.0 - 1e-3, rel=1e-15)  # (gap: to another hittable's root)
    assert e.albedo.tolist() == [0.5, 0.5, 0.5]
    # tmax exactly on the root: inclusive, and ambiguous for the kernel (the root rounds); just below it: a miss
    e = _one(sd, _ray((0, 0, 0), (0, 0, -1), tmax=4.0))
    assert e.winner[1] == 0 and e.range_margin == 0.0 and not unambiguous(e)
    e = _one(sd, _ray((0, 0, 0), (0, 0, -1), tmax=float(np.nextafter(4.0, 0.0))))
    assert e.winner is None and e.roots == []
    # from the centre: the far root 1, outward normal (0, 0, -1), back face
    e = _one(sd, _ray((0, 0, -5), (0, 0, -1)))
    assert float(e.winner[0].val) == 1.0 and e.normal.tolist() == [0.0, 0.0, -1.0] and not e.front_face
    # tangent: the double root 5, once; (p - c)·d = 0 is not a front face
    e = _one(sd, _ray((1, 0, 0), (0, 0, -1)))
    assert [(float(x.val), j) for x, j in e.roots] == [(5.0, 0)] and not e.front_face and e.disc_margin == 0.0
    assert not unambiguous(e)
    # pointing away; and tmin past the near root with tmax between the roots
    assert _one(sd, _ray((0, 0, 0), (0, 0, 1))).winner is None
    assert _one(sd, _ray((0, 0, 0), (0, 0, -1), tmax=5.0), tmin=4.5).winner is None
    assert float(_one(sd, _ray((0, 0, 0), (0, 0, -1), tmax=5.0)).winner[0].val) == 4.0
    # an irrational root: 1 + √3 / 2 off-axis, exact comparisons against tmax on either side of it
    e = _one(sd, _ray((0.5, 0, 0), (0, 0, -1)))
    x = e.winner[0]
    assert x.s == -1 and x.P == 5 and x.Q == Fraction(3, 4)
    f = float(x.val)
    below = float(np.nextafter(f, 0.0)) if x.le(Fraction(f)) else f  # the largest double below the root, and the next one up
    above = float(np.nextafter(below, 9.0))
    assert _one(sd, _ray((0.5, 0, 0), (0, 0, -1), tmax=below)).winner is None
    assert _one(sd, _ray((0.5, 0, 0), (0, 0, -1), tmax=above)).winner[1] == 0
    # two identical spheres: the larger index, and both roots listed
    e = _one(_pool([s0, s0]), _ray((0, 0, 0), (0, 0, -1)))
    assert e.winner[1] == 1 and [j for _, j in e.roots] == [1, 0, 1, 0]
    # a triangle at the sphere's near root: equal t, the triangle (larger index) wins
    tri_tie = ((-1.0, -1.0, -4.0), (1.0, -1.0, -4.0), (0.0, 1.0, -4.0))
    e = _one(_pool([s0], [tri_tie]), _ray((0, 0, 0), (0, 0, -1)))
    assert e.winner[1] == 1 and float(e.winner[0].val) == 4.0 and e.gap == 0.0


def test_exact_reference_triangle_records():
    # e1 = (2, 0, 0), e2 = (1, 2, 0): cross(e1, e2) = (0, 0, 4), the outward normal +z
    tri = ((-1.0, -1.0, -3.0), (1.0, -1.0, -3.0), (0.0, 1.0, -3.0))
    sd = _pool([], [tri])
    e = _one(sd, _ray((0, 0, 0), (0, 0, -1)))  # from the +z side: front face
    assert e.winner[1] == 0 and float(e.winner[0].val) == 3.0 and e.normal.tolist() == [0.0, 0.0, 1.0] and e.front_face
    assert e.point.tolist() == [0.0, 0.0, -3.0] and e.bary_margin == 0.25 and unambiguous(e)
    e = _one(sd, _ray((0, 0, -10), (0, 0, 2)))  # from behind: the same outward normal, a back face, t = 3.5
    assert float(e.winner[0].val) == 3.5 and e.normal.tolist() == [0.0, 0.0, 1.0] and not e.front_face
    # on the edge v0-v1 (barycentric 0 exactly) and on the vertex v2: hits, with no margin
    for target in ((0.0, -1.0, -3.0), (0.0, 1.0, -3.0), (1.0, -1.0, -3.0)):
        e = _one(sd, _ray((0, 0, 0), target))
        assert e.winner is not None and float(e.winner[0].val) == 1.0 and e.bary_margin == 0.0, target
        assert e.point.tolist() == list(target)
    # just outside the edge: a miss
    assert _one(sd, _ray((0, 0, 0), (0.0, float(np.nextafter(-1.0, -2.0)), -3.0))).winner is None
    # parallel to the plane: no root
    assert _one(sd, _ray((0, 0, -3), (1, 0, 0))).winner is None


@pytest.mark.parametrize("precision", [F32, F64])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_mode_b_within_the_exact_bounds(oracle, name, precision):
    """The mode-B brute force — what the query kernels match bit for bit — against the exact reference: the winner wherever it is
    unambiguous, t, and for sphere winners point, normal and front_face within the stated bounds; material exact."""
    t = SCENES[name]()
    sd = t.scene_desc()
    rays = ray_mix(oracle, t, precision, 256, seed=sum(map(ord, name)) + precision)
    S = Scene(sd)
    ex = exact_find_hit(sd, rays, TMIN, precision, S)
    idx, tt, rec, _ = brute_force(oracle, sd, rays, TMIN, precision)
    got = {"index": idx, "t": tt, "material": np.where(idx >= 0, S.mat[np.maximum(idx, 0)], -1), "point": rec[:, 2:5],
           "normal": rec[:, 5:8], "front_face": rec[:, 8], "record": idx < sd.n_spheres}
    summary = check_exact(sd, rays, got, ex, precision, S)
    print(name, precision, summary)
    assert summary["unambiguous"] >= 0.8


def _header_bounds():
    h = open(os.path.join(ROOT, "include", "rayz_hip.h")).read()
    lo = float(re.search(r"#define RAYZ_QUERY_MIN_DIR (\S+)", h).group(1))
    hi = float(re.search(r"#define RAYZ_QUERY_MAX_DIR (\S+)", h).group(1))
    return lo, hi


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _aimed(rng, o, target):
    """Directions from o to target scaled by a power of two so that max_k |d_k| lies in [1, 2)."""
    d = target - o
    return d / 2.0 ** np.floor(np.log2(np.abs(d).max(axis=1, keepdims=True)))


def _records(rng, piece, precision, n=1500):
    """(records, direction columns, [tmin, tmax] columns) of random rays aimed into random spheres (all velocity classes),
    triangles or boxes (both node formats); f32 rays for F32."""
    rec = np.zeros((n, capi.KAT_IN_STRIDE))
    o = rng.uniform(-20, 20, (n, 3))
    if piece == "sphere":
        c, r, tm = rng.uniform(-5, 5, (n, 3)), rng.uniform(0.1, 2, n), rng.choice([0.0, 0.5, 1.0], n)
        cls = rng.integers(0, 3, n)
        v = np.where((cls == 0)[:, None], 0.0, np.where((cls == 1)[:, None], [0, 1, 0] * rng.uniform(-1, 1, (n, 1)),
                                                         rng.uniform(-1, 1, (n, 3))))
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        target = c + v * tm[:, None] + u * (r * rng.uniform(0, 1, n))[:, None]
        rec[:, 0:3], rec[:, 3:6], rec[:, 6], rec[:, 7:10], rec[:, 10:13], rec[:, 13] = c, v, r, o, _aimed(rng, o, target), tm
        dcol, tcol = slice(10, 13), (14, 15)
    elif piece == "triangle":
        v0 = rng.uniform(-5, 5, (n, 3))
        v1, v2 = v0 + rng.normal(size=(n, 3)), v0 + rng.normal(size=(n, 3))
        b = rng.dirichlet([1, 1, 1], n)
        target = b[:, 0:1] * v0 + b[:, 1:2] * v1 + b[:, 2:3] * v2
        rec[:, 0:3], rec[:, 3:6], rec[:, 6:9], rec[:, 9:12], rec[:, 12:15] = v0, v1, v2, o, _aimed(rng, o, target)
        dcol, tcol = slice(12, 15), (15, 16)
    else:
        lo = rng.uniform(-5, 5, (n, 3))
        hi = lo + rng.uniform(0.01, 3, (n, 3))
        rec[:, 0:3], rec[:, 3:6] = _f32(lo), _f32(hi)
        rec[:, 6:9], rec[:, 9:12], rec[:, 26] = o, _aimed(rng, o, rng.uniform(lo, hi)), rng.integers(0, 2, n)
        dcol, tcol = slice(9, 12), (12, 13)
    rec[:, tcol[0]], rec[:, tcol[1]] = TMIN, np.inf
    if precision == F32:
        first = 7 if piece == "sphere" else (9 if piece == "triangle" else 6)
        rec[:, first:dcol.stop] = _f32(rec[:, first:dcol.stop])
        rec[:, tcol[0]] = _f32(TMIN)
    return rec, dcol, tcol


_OPS = {"sphere": capi.KAT_SPHERE_HIT, "triangle": capi.KAT_TRIANGLE_HIT, "box": capi.KAT_BOX_HIT}


def _scaled(oracle, rec, dcol, tcol, op, precision, k):
    r2 = rec.copy()
    r2[:, dcol] *= 2.0 ** k
    r2[:, tcol[0]] *= 2.0 ** -k
    r2[:, tcol[1]] *= 2.0 ** -k
    return oracle.kat_b(op, r2, precision)


@pytest.mark.parametrize("precision", [F32, F64])
@pytest.mark.parametrize("piece", sorted(_OPS))
def test_mode_b_pieces_are_scale_covariant_over_the_accepted_directions(oracle, piece, precision):
    """findHit does not depend on the scale of d: with d·2^k and tmin, tmax·2^-k every piece must take the same decisions and
    return t·2^-k exactly.  Swept from 2^16 below RAYZ_QUERY_MIN_DIR to 2^16 above RAYZ_QUERY_MAX_DIR (max_k |d_k| of the base rays
    lies in [1, 2)); most rays hit, so a lost hit shows."""
    lo, hi = _header_bounds()
    assert lo == 2.0 ** -32 and hi == 2.0 ** 32
    rng = np.random.default_rng(7 + precision)
    rec, dcol, tcol = _records(rng, piece, precision)
    op = _OPS[piece]
    base = oracle.kat_b(op, rec, precision)
    assert (base[:, 0] == 1).mean() > 0.9
    ks = sorted(set(range(-48, 49, 8)) | {-33, -32, 31, 32, 47})
    for k in ks:
        out = _scaled(oracle, rec, dcol, tcol, op, precision, k)
        assert np.array_equal(out[:, 0], base[:, 0]), (k, int((out[:, 0] != base[:, 0]).sum()), "decisions changed")
        h = base[:, 0] == 1
        assert np.array_equal(out[h, 1] * 2.0 ** k, base[h, 1]), (k, "t is not scaled exactly")


def test_directions_beyond_the_margin_do_lose_hits(oracle):
    """Why the range is refused beyond its ends: the first scales at which the pieces lose true hits (the refusal keeps 2^16 or
    more from each of them): the F32 sphere filter and triangle test beyond 2^60 (d·d, det² overflow f32), the box test below
    2^-60 (1/d_k capped at 2^64), the F64 box test beyond 2^100 (d_k held to ±2^100)."""
    rng = np.random.default_rng(5)
    for piece, precision, k in [("sphere", F32, 64), ("triangle", F32, 64), ("box", F32, -64), ("box", F64, -64),
                                ("box", F64, 104)]:
        rec, dcol, tcol = _records(rng, piece, precision)
        base = oracle.kat_b(_OPS[piece], rec, precision)
        out = _scaled(oracle, rec, dcol, tcol, _OPS[piece], precision, k)
        lost = ((base[:, 0] == 1) & (out[:, 0] != 1)).mean()
        assert lost > 0.1, (piece, precision, k, lost)
