"""Speed buckets of the flat list's y-moving plane runs on the device.

1. The bucket form itself: RAYZ_KAT_BUCKET_DISCS runs ScanGroup<float, 5>::discs with the bucket's K2 put in the basis as
   scan_plane_class does, on the padded r2b the library makes.  Held bit for bit to an f32 evaluation in numpy written here (f32
   kernel; the FMAs rounded once, see fma32) and to the CPU mirror (tests/bucket_mirror.cpp `discs`, both precisions); r2b to the
   rule restated here; and no sphere whose f64 discriminant is >= 0 is rejected.
2. Bucket layouts rendered: runs of 64, 71, 72, 73 and 200 members of one speed, a spread too wide for any bucket, negative and
   mixed-sign speeds, two runs with several buckets each, heights at 3e4, a row of overlapping spheres inside one bucket (more
   candidates than a lane parks), and one DeviceScene re-padded for a far camera.  Each scene first asserts, through the mirror's
   `layout`, that it forms the buckets it was built for; then the flat list is held to oracle mode B bit for bit, segments
   included, and to the device's BVH frame, in f32 and f64 (tests/test_plane_runs_gpu.py: check_frames)."""
import subprocess

import numpy as np
import pytest

import kat_records as K
from rayz_amd import capi
from test_plane_runs import _run, _spheres, _write, mirror  # noqa: F401  (mirror: a fixture)
from test_plane_runs_gpu import Scene, check_frames
from test_speed_buckets import bmirror, bucket_sizes, check_layout  # noqa: F401  (bmirror: a fixture)

pytestmark = pytest.mark.gpu

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR = capi.TRAVERSAL_LINEAR
BUCKET = capi.KAT_BUCKET_DISCS
f32 = np.float32


# ---- 1. the bucket form ----------------------------------------------------------------------------------------------------
def fma32(a, b, c):
    """fl32(a·b + c) for f32 arrays, rounded once: the product of two f32 is exact in f64; the f64 sum is rounded to odd
    (its error recovered by two-sum), after which the rounding to f32 is the rounding of the exact value."""
    p = np.float64(a) * np.float64(b)
    c = np.float64(c)
    with np.errstate(invalid="ignore", over="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
    fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
    up = np.nextafter(s, np.inf)
    dn = np.nextafter(s, -np.inf)
    s = np.where(fix, np.where(err > 0, up, dn), s)
    return s.astype(f32)


def bucket_discs_f32(rec):
    """The f32 kernel's bucket form of a RAYZ_KAT_BUCKET_DISCS record (r2b at [28..31]): device_math.hpp's unit, flat_scan.hpp's make_basis,
    bucket_k2 and ScanGroup<float, 3>::discs, operation by operation."""
    d = f32(rec[:, 23:26])
    o = f32(rec[:, 20:23])
    m = np.sqrt(fma32(d[:, 2], d[:, 2], fma32(d[:, 1], d[:, 1], d[:, 0] * d[:, 0])))
    inv = f32(1) / m
    ux, uy, uz = d[:, 0] * inv, d[:, 1] * inv, d[:, 2] * inv
    h2 = fma32(uz, uz, ux * ux)
    big = h2 > f32(1e-30)
    with np.errstate(divide="ignore", invalid="ignore"):
        ih = f32(1) / np.sqrt(h2)
    e1x = np.where(big, uz * ih, f32(1))
    e1z = np.where(big, -(ux * ih), f32(0))
    e2x = uy * e1z
    e2y = fma32(uz, e1x, -(ux * e1z))
    e2z = -(uy * e1x)
    k1 = -fma32(o[:, 2], e1z, o[:, 0] * e1x)
    k2 = -fma32(o[:, 2], e2z, fma32(o[:, 1], e2y, o[:, 0] * e2x))
    K2 = fma32(f32(rec[:, 27]), f32(rec[:, 26]) * e2y, fma32(f32(rec[:, 4]), e2y, k2))
    out = np.empty((len(rec), 4), f32)
    for k in range(4):
        cx, cz, r2b = f32(rec[:, k]), f32(rec[:, 8 + k]), f32(rec[:, 28 + k])
        p1 = fma32(cz, e1z, fma32(cx, e1x, k1))
        p2 = fma32(cz, e2z, fma32(cx, e2x, K2))
        out[:, k] = fma32(-p1, p1, fma32(-p2, p2, r2b))
    return out, K2


def bucket_pad_r2(rec, precision):
    """rayz_hip.hip: pad_radius2_bucket — the pad rule of scan_pad_r2 for the sphere of radius r + h and speed |vy| + h,
    h = |vy − v0| (against the f64 and the f32 speed) nudged up."""
    norm = lambda x, y, z: np.sqrt(x * x + y * y + z * z)  # noqa: E731
    vy, v0, r = rec[:, 16:20], np.float64(f32(rec[:, 27]))[:, None], np.abs(rec[:, 12:16])
    cn = norm(rec[:, 0:4], rec[:, 4:5], rec[:, 8:12]) + norm(0.0, vy, 0.0) + r
    S = np.maximum(norm(rec[:, 20], rec[:, 21], rec[:, 22]), cn.max(1))
    h = np.maximum(np.abs(vy - v0), np.abs(np.float64(f32(vy)) - v0)) * (1.0 + 2.0 ** -50) + 1e-300
    E = (32.0 if precision == F32 else 40.0) * 5.9604644775390625e-08 * (norm(rec[:, 0:4], rec[:, 4:5], rec[:, 8:12]) + norm(0.0, vy, 0.0) + h + r + h + S[:, None])
    v = (r + h + E) ** 2
    f = v.astype(f32)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, f32(np.inf)), f).astype(np.float64)


def bucket_blocks(rng, n):
    """random_plane_blocks' y-moving records (one f32 height per block, small / negative / ±0 / 3e4 heights, grazing and level
    rays) as blocks of ONE bucket: the four speeds within r_min / 16 of the bucket's v0 (half of them at the full distance)."""
    rec = K.random_plane_blocks(rng, 2 * n)
    rec = rec[rec[:, 27] == 3.0][:n]
    v0 = K.f32r(rng.uniform(-0.5, 0.5, len(rec)))
    h = rec[:, 12:16].min(1) / 16 * np.where(rng.random(len(rec)) < 0.5, 1.0, rng.random(len(rec)))
    rec[:, 16:20] = K.f32r(v0[:, None] + h[:, None] * rng.choice([-1.0, 1.0], (len(rec), 4)) * np.where(rng.random((len(rec), 4)) < 0.5, 1.0, rng.random((len(rec), 4))))
    # aim again at sphere 0 where it is at the ray's time, near its rim for half the records
    t = rec[:, 26]
    tgt = np.stack([rec[:, 0], rec[:, 4] + rec[:, 16] * t, rec[:, 8]], 1)
    off = K.unit(rng.normal(size=(len(rec), 3))) * (rec[:, 12] * np.where(rng.random(len(rec)) < 0.5, 1.0 + rng.uniform(-1e-4, 1e-4, len(rec)), rng.uniform(0, 2.0, len(rec))))[:, None]
    keep = np.abs(rec[:, 24]) > 1e-2 * np.linalg.norm(rec[:, 23:26], axis=1)  # leave the grazing and level rays as they are
    rec[keep, 23:26] = K.f32r((tgt + off - rec[:, 20:23]) * rng.uniform(0.3, 3.0, (len(rec), 1)))[keep]
    rec[:, 27], rec[:, 32] = v0, 0.0
    return rec


def f64_disc(rec):
    """The reference's discriminant in f64 (narrow_eval's) for the record's four spheres against its ray, and which of its
    signs are beyond the rounding of this evaluation."""
    o, d, t = rec[:, 20:23], rec[:, 23:26], rec[:, 26]
    out, clear = np.empty((len(rec), 4)), np.empty((len(rec), 4), bool)
    for k in range(4):
        q = np.stack([rec[:, k] - o[:, 0], rec[:, 4] + rec[:, 16 + k] * t - o[:, 1], rec[:, 8 + k] - o[:, 2]], 1)
        a, hb, cc = (d * d).sum(1), (d * q).sum(1), (q * q).sum(1) - rec[:, 12 + k] ** 2
        out[:, k] = hb * hb - a * cc
        clear[:, k] = np.abs(out[:, k]) > 1e-11 * (hb * hb + a * ((q * q).sum(1) + rec[:, 12 + k] ** 2))
    return out, clear


@pytest.mark.parametrize("prec", [F32, F64])
def test_device_bucket_form(gpu, bmirror, tmp_path, prec):
    rec = bucket_blocks(np.random.default_rng(12), 60_000)
    if prec == F32:
        rec[:, 20:27] = K.f32r(rec[:, 20:27])
    got = gpu.kat(BUCKET, rec, prec)
    assert np.array_equal(got[:, 8:12], bucket_pad_r2(rec, prec))
    r = rec.copy()
    r[:, 28:32] = got[:, 8:12]
    p = _write(tmp_path, "rec.bin", r)
    run = subprocess.run([bmirror, "discs", str(p), str(int(prec == F64))], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr
    m = np.frombuffer(run.stdout, dtype=f32).reshape(-1, 9)
    bits = lambda x: np.asarray(x, dtype=f32).view(np.uint32)  # noqa: E731
    assert np.array_equal(bits(got[:, :4]), bits(m[:, :4])) and np.array_equal(bits(got[:, 4]), bits(m[:, 8]))
    assert not (m[:, 4:8] >= 0).any()  # a pad slot (r2b = -inf) at any place of the block never passes
    if prec == F32:
        want, K2 = bucket_discs_f32(r)
        assert np.array_equal(bits(got[:, 4]), bits(K2))
        same = bits(got[:, :4]) == bits(want)
        assert same.all(), (int((~same).any(1).sum()), np.flatnonzero(~same.any(1))[:5].tolist())
    # conservative: decided on the ray the kernel traces (narrowed to f32 for the f32 kernel above)
    disc, clear = f64_disc(rec)
    hit = (disc >= 0) & clear
    assert hit.sum() > 10_000 and (got[:, :4][hit] >= 0).all(), int((got[:, :4][hit] < 0).sum())
    assert 0.05 < (got[:, :4] >= 0).mean() < 0.7
    with pytest.raises(capi.RayzHipError, match="v0"):
        bad = rec[:4].copy()
        bad[1, 27] = np.inf
        gpu.kat(BUCKET, bad, prec)


# ---- 2. bucket layouts rendered --------------------------------------------------------------------------------------------
def bucket_group(s, cy, n, vy, spread=8.0, r=(0.2, 0.45)):
    """n y-moving spheres at one height; vy() draws each speed."""
    for _ in range(n):
        y = cy if s.y0 == 0 else s.y0 + cy
        s.sphere((s.rng.uniform(-spread, spread), y, s.rng.uniform(-spread, spread)), s.rng.uniform(*r), (0.0, float(vy()), 0.0))
    return s


def _bucket_layout(name):
    """(scene, bucket sizes per mov-Y run it must form)."""
    if name == "sizes_64_71_72_73":  # one speed per run: one bucket each, the rest and the pads in the run's 4-field blocks
        s = Scene(40)
        for h, n, v in [(0.4, 64, 0.3), (1.3, 71, -0.25), (2.2, 72, 0.45), (3.1, 73, 0.1)]:
            bucket_group(s, h, n, lambda v=v: v)
        return s.loose(), [[64], [64], [72], [72]]
    if name == "size_200_nearly_one_speed":
        s = Scene(41)
        bucket_group(s, 0.8, 200, lambda: s.rng.uniform(0.30, 0.32), spread=6.0)
        return s.loose(), [[200]]
    if name == "wide_spread_no_bucket":
        s = Scene(42)
        bucket_group(s, 0.8, 120, lambda: s.rng.uniform(-0.6, 0.6))
        return s.loose(), [[]]
    if name == "mixed_sign":  # a bucket of negative speeds, one across zero, one of positive speeds, and spheres left over
        s = Scene(43)
        bucket_group(s, 0.6, 72, lambda: s.rng.uniform(-0.41, -0.39))
        bucket_group(s, 0.6, 80, lambda: s.rng.choice([-1.0, 1.0]) * s.rng.uniform(1e-5, 0.01))
        bucket_group(s, 0.6, 66, lambda: s.rng.uniform(0.39, 0.41))
        bucket_group(s, 0.6, 12, lambda: s.rng.uniform(0.6, 0.9))
        return s.loose(), [[72, 80, 64]]
    if name == "two_runs":
        s = Scene(44)
        bucket_group(s, 0.5, 70, lambda: s.rng.uniform(0.2, 0.22)), bucket_group(s, 0.5, 90, lambda: s.rng.uniform(0.5, 0.52))
        bucket_group(s, 1.9, 130, lambda: s.rng.uniform(-0.31, -0.30))
        s.group(0, 1.2, 70)  # and a static run beside them
        return s.loose(), [[64, 88], [128]]
    if name == "far_3e4":
        y0 = 3.0e4
        s = Scene(45, look_from=(0.0, y0 + 6.0, 14.0), look_at=(0.0, y0 + 1.0, 0.0), y0=y0)
        bucket_group(s, 1.0, 100, lambda: s.rng.uniform(0.25, 0.27))
        return s.loose(), [[96]]
    if name == "row_view":  # along a row of overlapping spheres of one bucket: more than 4 candidates per lane inside it
        s = Scene(46, look_from=(-12.0, 1.0, 0.0), look_at=(10.0, 1.0, 0.0), width=32)
        for k in range(96):
            s.sphere((-4.0 + 0.12 * k, 1.0, 0.15 * np.sin(k)), 0.45, (0.0, 0.2 + 1e-4 * (k % 7), 0.0))
        return s.loose(), [[96]]
    raise KeyError(name)


BUCKET_LAYOUTS = ["sizes_64_71_72_73", "size_200_nearly_one_speed", "wide_spread_no_bucket", "mixed_sign", "two_runs", "far_3e4",
                  "row_view"]


def assert_buckets(mirror, bmirror, tmp_path, t, want):
    lay = check_layout(mirror, bmirror, tmp_path, _spheres(t))
    assert bucket_sizes(lay) == want, bucket_sizes(lay)


@pytest.mark.parametrize("name", BUCKET_LAYOUTS)
def test_bucket_layout_renders_like_the_oracle(gpu, oracle, mirror, bmirror, tmp_path, name):
    s, want = _bucket_layout(name)
    t = s.build()
    assert_buckets(mirror, bmirror, tmp_path, t, want)
    check_frames(gpu, oracle, t, name)


def test_device_scene_with_buckets_through_near_far_near(gpu, oracle, mirror, bmirror, tmp_path):
    """One DeviceScene with buckets: near camera, a camera 20,000 units out (the larger origin bound re-pads the streams, the
    buckets' r2b with them), near again; f32 and f64; every step held to the oracle."""
    from test_reuse_gpu import FAR, Want, camera, params, render_checked

    s, want = _bucket_layout("two_runs")
    t = s.build()
    assert_buckets(mirror, bmirror, tmp_path, t, want)
    scene = t.scene_desc()
    w = Want(oracle, scene)
    near = camera(oracle, ((0.0, 7.0, 15.0), 40.0, 10.0), 48, 27)
    far = camera(oracle, FAR, 64, 36)
    ds = gpu.DeviceScene(scene)
    try:
        for prec in (F32, F64):
            for cam, wh, tag in ((near, (48, 27), "near"), (far, (64, 36), "far"), (near, (48, 27), "near again")):
                p = params(t.params(), width=wh[0], height=wh[1], traversal=LINEAR, precision=prec)
                render_checked(ds, w, cam, p, f"{tag}, precision {prec}")
    finally:
        ds.close()
