"""The flat list's reject test in its XY basis (e1 in the xy-plane: DESIGN.md §4.3; flat_scan.hpp: kBasisXY; trace_kernels_flat.hpp: flat_xy_kernel) and the
host's choice between the two bases (rayz_amd/csrc/plane_runs.hpp: scan_price).  CPU checks through a C++ mirror built here
(tests/flat_xy_mirror.cpp: the device's forms written with fmaf, and the library's own plane_runs.hpp):
  * 0 false negatives against the f64 discriminant, with f32 rays and with f64 rays narrowed, every sphere in the form its place
    in the layout gives it (run and bucket: 5 FMAs, mov-Y remainder: 7, loose: 7 / 9, general velocity: 12): config 3's segments
    against its whole pool; the adversarial records of tests/kat_records.py, also at heights ±0, negative and 3e4, each sphere in
    every form its class can take, buckets the whole r / 16 off the member's speed; bucket pools of mixed-sign speeds at times 0,
    1 and random; and the rays the XZ basis never needed: ud.x = ud.y = 0 exactly, |ud.x|, |ud.y| about 1e-16 with h² below and
    just above 1e-30, rays parallel to y, parallel to x, and in the plane y = cy;
  * tightness: on config 3's segments the XY forms pass at most 1.01x the candidates of the XZ forms on the same pairs;
  * the pricing rule: runs only -> XY; loose y-moving spheres only -> XZ; no run -> XZ; a tie -> XZ."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import kat_records as K
from test_plane_runs import _config3_segments, _groups, _run, _write
from test_speed_buckets import aimed_rays, pool, spread

HERE = os.path.dirname(os.path.abspath(__file__))
XZ, XY = 1, 2  # plane_runs.hpp: kScanFormXZ, kScanFormXY


@pytest.fixture(scope="module")
def xmirror(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("flat_xy") / "flat_xy_mirror")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "flat_xy_mirror.cpp")],
                   check=True, capture_output=True, timeout=300)
    return exe


def bound(sph, rays):
    return max(np.max(np.linalg.norm(sph[:, 0:3], axis=1) + np.linalg.norm(sph[:, 3:6], axis=1) + np.abs(sph[:, 6])),
               np.max(np.linalg.norm(rays[:, 0:3], axis=1))) * (1 + 1e-3)


def clean(au, what):
    assert au["false_negatives"] == 0 and au["pad_passes"] == 0, (what, au)
    assert au["parent_false_negatives"] == 0, (what, au)  # (the XZ forms on the same pairs: the mirror's own sanity)


# ---- config 3: conservative and tight ----------------------------------------------------------------------------------------
def test_config3_segments_no_false_negative_and_as_tight_as_the_xz_forms(xmirror, tmp_path):
    sph, rays, S = _config3_segments(np.random.default_rng(5))
    sp, rp = _write(tmp_path, "s.bin", sph), _write(tmp_path, "r.bin", rays)
    lay = _run(xmirror, tmp_path, "form", sp)
    print("config 3 layout", lay)
    assert lay["form"] == XY and lay["slots"]["plane_static"] + lay["slots"]["bucket"] > 9900 and lay["slots"]["loose_movy"] == 0
    for f64_rays in (0, 1):
        au = _run(xmirror, tmp_path, "audit", sp, rp, repr(S), f64_rays)
        print("xy-form audit, config 3,", "f64 rays" if f64_rays else "f32 rays", au)
        assert au["pairs"] == len(rays) * len(sph) and au["f64_hits"] > 10_000, au
        clean(au, "config 3")
        assert au["f64_hits"] <= au["candidates"], au
        assert au["candidates"] <= 1.01 * au["parent_candidates"], au


# ---- adversarial pairs, every form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("height", [None, 0.0, -0.0, -7.25, 3.0e4])
def test_adversarial_records_in_every_form_their_class_can_take(xmirror, tmp_path, height):
    """kat_records' (ray, sphere) pairs (grazing, far origins, big coordinates), as they are (None) or moved in y so that the sphere
    sits at `height`: the sphere as its own run / loose / general, a y-moving one also in a bucket the whole r / 16 off its speed."""
    rng = np.random.default_rng(9)
    rec = K.random_sphere_hits(rng, 40_000, big=True)
    if height is not None:
        dy = height - rec[:, 1]
        rec[:, 1] = height
        rec[:, 8] = K.f32r(rec[:, 8] + dy)
    rec[:, 0:3], rec[:, 7:10] = K.f32r(rec[:, 0:3]), K.f32r(rec[:, 7:10])
    sph, rays = rec[:, 0:7], rec[:, 7:14]
    S = bound(sph, rays)
    for f64_rays in (0, 1):
        au = _run(xmirror, tmp_path, "pairs", _write(tmp_path, "s.bin", sph), _write(tmp_path, "r.bin", rays), repr(S), f64_rays)
        assert au["pairs"] > 2 * len(rec) and au["f64_hits"] > 20_000, au
        clean(au, (height, f64_rays))


# ---- buckets: mixed-sign speeds, times 0 / 1 / random --------------------------------------------------------------------------
@pytest.mark.parametrize("y0", [0.0, -6.5, 3.0e4])
def test_bucket_pools_of_mixed_sign_speeds(xmirror, tmp_path, y0):
    rng = np.random.default_rng(11)
    around_zero = lambda n: rng.choice([-1.0, 1.0], n) * rng.uniform(1e-6, 0.008, n)  # noqa: E731  (one bucket across the sign)
    sph = pool([(0.2, 400, spread(0.2, 0.26, rng)), (1.0, 160, spread(-0.31, -0.30, rng)), (1.8, 96, around_zero)], rng, r=(0.15, 0.3), y0=y0)
    rays = aimed_rays(sph[sph[:, 4] != 0], rng, 4000)  # times 0, 1 and random; a third of the rays level with their target
    S = bound(sph, rays)
    sp, rp = _write(tmp_path, "s.bin", sph), _write(tmp_path, "r.bin", rays)
    lay = _run(xmirror, tmp_path, "form", sp)
    assert lay["buckets"] >= 4 and lay["slots"]["plane_movy"] > 0 and lay["slots"]["loose_movy"] > 0 and lay["slots"]["loose_static"] > 0, lay
    for f64_rays in (0, 1):
        au = _run(xmirror, tmp_path, "audit", sp, rp, repr(S), f64_rays)
        assert au["pairs"] == len(rays) * len(sph) and au["f64_hits"] > 2000, au
        clean(au, (y0, f64_rays))


# ---- the rays the XZ basis never needed ------------------------------------------------------------------------------------------
def special_rays(sph, rng, per_kind=600):
    """Rays aimed at points at distance u·r of a sphere's centre at the ray's time (u within 1e-3 of the rim for half of them), from
    near and far, along directions that reach the XY basis's corners:
      0  ud.x = ud.y = 0 exactly (along ±z: the fallback e1 = (1, 0, 0));
      1  |d.x|, |d.y| about 1e-16 beside d.z = ±1: h² about 1e-32, the fallback;
      2  h² just above 1e-30 (|d.x| = 1.0000001e-15 .. 1.1e-15, d.y below it): the smallest h the general branch divides by;
      3  parallel to y; 4  parallel to x (e1 = (0, ∓1, 0));
      5  in the plane y = cy of the target: o.y = cy exactly, d.y = 0."""
    out = []
    for kind in range(6):
        n = per_kind
        k = rng.integers(0, len(sph), n)
        time = np.select([np.arange(n) % 3 == 0, np.arange(n) % 3 == 1], [0.0, 1.0], rng.random(n))
        sgn = rng.choice([-1.0, 1.0], n)
        d = np.zeros((n, 3))
        if kind in (0, 1, 2):
            d[:, 2] = sgn
            if kind == 1:
                d[:, 0], d[:, 1] = rng.choice([-1.0, 1.0], n) * rng.uniform(0.5e-16, 2e-16, n), rng.choice([-1.0, 1.0], n) * rng.uniform(0.5e-16, 2e-16, n)
            if kind == 2:
                d[:, 0] = rng.choice([-1.0, 1.0], n) * 1e-15 * rng.uniform(1.0000001, 1.1, n)
                d[:, 1] = rng.choice([-1.0, 0.0, 1.0], n) * rng.uniform(0, 1e-16, n)
        elif kind == 3:
            d[:, 1] = sgn
        elif kind == 4:
            d[:, 0] = sgn
        else:
            a = rng.uniform(0, 2 * np.pi, n)
            d[:, 0], d[:, 2] = np.cos(a), np.sin(a)
        u = np.where(rng.random(n) < 0.5, 1.0 + rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-7, -3, n), rng.uniform(0, 1.3, n))
        dn = d / np.linalg.norm(d, axis=1, keepdims=True)
        if kind == 5:  # the offset in the plane too
            off = np.stack([-dn[:, 2], np.zeros(n), dn[:, 0]], 1) * rng.choice([-1.0, 1.0], (n, 1))
        else:
            off = rng.normal(size=(n, 3))
            off -= (off * dn).sum(1, keepdims=True) * dn
            off /= np.linalg.norm(off, axis=1, keepdims=True)
        c = sph[k, 0:3] + sph[k, 3:6] * time[:, None]
        o = c + off * (np.abs(sph[k, 6]) * u)[:, None] - dn * np.where(rng.random(n) < 0.5, rng.uniform(1, 3, n), rng.uniform(30, 60, n))[:, None]
        if kind == 5:
            o[:, 1] = sph[k, 1]
        out.append(np.concatenate([o, d * rng.choice([0.5, 1.0, 2.0], (n, 1)), time[:, None]], 1))
    return np.concatenate(out)


def test_special_rays_reach_both_branches_of_the_basis(xmirror, tmp_path):
    rng = np.random.default_rng(21)
    for y0 in (0.0, -3.0):
        sph = np.concatenate([pool([(0.4, 200, spread(0.30, 0.32, rng)), (1.2, 90, spread(-0.6, 0.6, rng))], rng, y0=y0),
                              _groups([(0, y0 + 0.4, 130), (0, y0 - 0.0, 70)], rng)])
        g = np.zeros((12, 7))  # and spheres of general velocity
        g[:, 0:3], g[:, 3:6], g[:, 6] = rng.uniform(-6, 6, (12, 3)) + [0, y0, 0], rng.uniform(-0.5, 0.5, (12, 3)), 0.4
        sph = np.concatenate([sph, g])
        rays = special_rays(sph, rng)
        # what the kinds are meant to reach, on the unit direction as the f32 kernel makes it
        d32 = np.float32(rays[:, 3:6])
        ud = d32 / np.sqrt(np.float32((np.float64(d32) ** 2).sum(1)))[:, None]
        h2 = np.float64(ud[:, 0]) ** 2 + np.float64(ud[:, 1]) ** 2
        n = len(rays) // 6
        assert (h2[:n] == 0).all() and (h2[n:2 * n] < 1e-30).all() and (h2[n:2 * n] > 0).all()
        assert (h2[2 * n:3 * n] > 1e-30).all() and (h2[2 * n:3 * n] < 1.3e-30).all()
        S = bound(sph, rays)
        sp, rp = _write(tmp_path, "s.bin", sph), _write(tmp_path, "r.bin", rays)
        lay = _run(xmirror, tmp_path, "form", sp)
        assert lay["runs"] == [2, 2] and lay["buckets"] >= 1 and all(v > 0 for v in lay["slots"].values()), lay
        for f64_rays in (0, 1):
            au = _run(xmirror, tmp_path, "audit", sp, rp, repr(S), f64_rays)
            print("xy-form audit, special rays,", "f64 rays" if f64_rays else "f32 rays", au)
            assert au["pairs"] == len(rays) * len(sph) and au["f64_hits"] > 3000, au
            clean(au, (y0, f64_rays))


# ---- the pricing rule ----------------------------------------------------------------------------------------------------------
def loose_movy(rng, n):
    s = np.zeros((n, 7))
    s[:, 0], s[:, 1], s[:, 2], s[:, 6] = rng.uniform(-9, 9, n), rng.uniform(-3, 3, n), rng.uniform(-9, 9, n), 0.3
    s[:, 4] = rng.uniform(0.1, 0.5, n)
    return s


def test_pricing_rule_on_small_pools(xmirror, tmp_path):
    rng = np.random.default_rng(3)
    form = lambda sph: _run(xmirror, tmp_path, "form", _write(tmp_path, "s.bin", sph))  # noqa: E731
    # runs only: one static run of 64, nothing else
    lay = form(_groups([(0, 0.5, 64)], rng))
    assert lay["slots"] == {"plane_static": 64, "bucket": 0, "plane_movy": 0, "loose_static": 0, "loose_movy": 0, "movg": 0}
    assert (lay["price_xz"], lay["price_xy"], lay["form"]) == (6 * 64, 5 * 64, XY)
    # a y-moving run of one speed: a bucket; still runs only
    one_speed = pool([(0.5, 64, lambda n: np.full(n, 0.3))], rng)
    lay = form(one_speed[(one_speed[:, 4] == 0.3)])
    assert lay["slots"]["bucket"] == 64 and lay["form"] == XY and lay["price_xy"] == 5 * 64
    # loose y-moving spheres only: 8 against 9
    lay = form(loose_movy(rng, 10))
    assert lay["slots"]["loose_movy"] == 16 and sum(lay["slots"].values()) == 16
    assert (lay["price_xz"], lay["price_xy"], lay["form"]) == (8 * 16, 9 * 16, XZ)
    # no run: loose static spheres (7 / 7) and general velocities (12 / 12) price alike: the XZ kernel stays
    s = _groups([(0, 0.5, 20), (0, 1.5, 30)], rng)
    g = loose_movy(rng, 3)
    g[:, 3] = 0.2
    lay = form(np.concatenate([s, g]))
    assert lay["runs"] == [0, 0] and lay["slots"]["movg"] == 4 and lay["price_xz"] == lay["price_xy"] == 7 * 56 + 12 * 4 and lay["form"] == XZ
    # a tie with a run in it: 64 plane slots save what 64 loose y-moving slots cost
    lay = form(np.concatenate([_groups([(0, 0.5, 64)], rng), loose_movy(rng, 64)]))
    assert lay["slots"]["plane_static"] == 64 and lay["slots"]["loose_movy"] == 64
    assert lay["price_xz"] == lay["price_xy"] == 896 and lay["form"] == XZ
    # one more plane pair tips it
    lay = form(np.concatenate([_groups([(0, 0.5, 72)], rng), loose_movy(rng, 64)]))
    assert lay["price_xy"] < lay["price_xz"] and lay["form"] == XY
    # the rule on bare slot counts: 6/5 plane and bucket, 7/7 mov-Y remainder and loose static, 8/9 loose mov-Y, 12/12 general
    for slots in ([1, 0, 0, 0, 0, 0], [0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 1, 0], [0, 0, 0, 0, 0, 1],
                  [0, 0, 0, 0, 0, 0], [3, 2, 7, 11, 5, 13], [3, 2, 7, 11, 6, 13], [1 << 40, 0, 0, 0, 1 << 40, 9]):
        pr = _run(xmirror, tmp_path, "price", *slots)
        ps, bk, pm, ls, lm, mg = slots
        assert pr["price_xz"] == 6 * (ps + bk) + 7 * (pm + ls) + 8 * lm + 12 * mg
        assert pr["price_xy"] == 5 * (ps + bk) + 7 * (pm + ls) + 9 * lm + 12 * mg
        assert pr["form"] == (XY if ps + bk > lm else XZ)
