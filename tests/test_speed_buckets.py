"""Speed buckets of the flat list's y-moving plane runs: run members of nearly one speed vy are tested
with ONE speed v0, folded into the ray's K2, against a radius grown by |vy − v0| — the static plane form, 6 packed FMAs per
sphere pair instead of 7.  CPU checks, through a C++ mirror built here (tests/bucket_mirror.cpp, which compiles the library's
own rayz_amd/csrc/plane_runs.hpp):
  * layout: every run member is in exactly one bucket or in the run's 4-field remainder; buckets are whole group pairs of at
    least 64 members, ordered by (f32 vy, pool index), with h = max |vy − v0| <= r_min / 16; the runs themselves — what the
    stream's head holds of them: count, plane slots, the PlaneRun records — are what plan_runs made before buckets existed
    (the existing mirror's `layout`); only the head's two spare words, which name the bucket section, are new;
  * the bucket form in f32 exactly as the kernel evaluates it passes every (ray, sphere, time) pair whose f64 discriminant is
    >= 0, pad slots never pass;
  * on config 3's own segments it lets through at most (1 + 1/16)² times the candidates of the parent's form (+ the 1000 of
    slack test_plane_runs.py grants);
  * the compiled f32 flat kernel has the bucket loop, 6·G/2 packed FMAs per group, after the four loops it had."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from rayz_amd import tracer
from test_plane_runs import G, ROOT, _config3_segments, _run, _spheres, _write, mirror  # noqa: F401  (mirror: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
CAP = 16  # plane_runs.hpp: kBucketCap
f32 = np.float32


@pytest.fixture(scope="module")
def bmirror(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("bucket") / "bucket_mirror")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "bucket_mirror.cpp")],
                   check=True, capture_output=True, timeout=300)
    return exe


def pool(spec, rng, r=(0.3, 0.3), y0=0.0):
    """Sphere rows for [(cy, members, vy sampler), ...]: y-moving groups as tests/test_plane_runs.py::_groups builds them (one
    height per group, x and z in ±9, radius 0.3 unless a range is given), the speeds drawn by the sampler; 20 static spheres and
    10 loose y-moving ones beside them; shuffled into one pool order."""
    rows = []
    for cy, n, vy in spec:
        s = np.zeros((n, 7))
        s[:, 0], s[:, 1], s[:, 2], s[:, 6] = rng.uniform(-9, 9, n), y0 + cy, rng.uniform(-9, 9, n), rng.uniform(*r, n)
        s[:, 4] = vy(n)
        rows.append(s)
    extra = np.zeros((30, 7))
    extra[:, 0], extra[:, 1], extra[:, 2], extra[:, 6] = rng.uniform(-9, 9, 30), y0 + rng.uniform(-3, 3, 30), rng.uniform(-9, 9, 30), 0.3
    extra[20:, 4] = rng.uniform(0.1, 0.5, 10)
    sph = np.concatenate(rows + [extra])
    return sph[rng.permutation(len(sph))]


def same(v):
    return lambda n: np.full(n, v)


def spread(lo, hi, rng):
    return lambda n: rng.uniform(lo, hi, n)


def check_layout(mirror, bmirror, tmp_path, sph):
    """The properties every bucket layout has; returns the bucket mirror's layout."""
    sp = _write(tmp_path, "s.bin", sph)
    lay = _run(bmirror, tmp_path, "layout", sp)
    parent = _run(mirror, tmp_path, "layout", sp)["classes"][1]
    # the runs: plan_runs' own, as the existing mirror reports them (head words 0 and 1 and the PlaneRun records)
    assert lay["plane_slots"] == parent["plane_slots"] and len(lay["runs"]) == len(parent["runs"])
    for r, p in zip(lay["runs"], parent["runs"]):
        assert (r["first"], r["end"], r["members"]) == (p["first"], p["end"], p["members"])
        assert r["cy_bits"] == int(f32(p["cy"]).view(np.uint32)) or p["cy"] == 0  # (the JSON prints -0 as an integer)
    vy32, rad = f32(sph[:, 4]), np.abs(sph[:, 6])
    for r in lay["runs"]:
        order, nb = r["order"], r["bucketed"]
        assert sorted(order) == r["members"]  # every member in exactly one place
        assert order[nb:] == sorted(order[nb:])  # the remainder in pool order
        at, last_hi = r["first"], -np.inf
        for b in r["buckets"]:
            n = b["end"] - b["first"]
            assert b["first"] == at and n % (2 * G) == 0 and n >= 64, b  # whole group pairs, back to back, no pads
            m = order[at - r["first"]:at - r["first"] + n]
            v = vy32[m]
            assert np.isfinite(v).all()
            key = list(zip(v.tolist(), m))
            assert key == sorted(key)  # by (f32 vy, pool index)
            assert v[0] >= last_hi  # and the buckets by speed
            last_hi = v[-1]
            v0 = np.uint32(b["v0_bits"]).view(f32)
            assert v0 == f32((np.float64(v[0]) + np.float64(v[-1])) * 0.5)  # the midpoint of the members' min and max
            h = np.max(np.abs(np.float64(v) - np.float64(v0)))
            assert h <= rad[m].min() / CAP, (h, rad[m].min())
            at = b["end"]
        assert at == r["first"] + nb and at <= r["end"] and r["end"] - r["first"] - len(order) < 2 * G
    return lay


def bucket_sizes(lay):
    return [[b["end"] - b["first"] for b in r["buckets"]] for r in lay["runs"]]


@pytest.mark.parametrize("n, want", [(64, [64]), (71, [64]), (72, [72]), (73, [72]), (200, [200])])
def test_run_sizes_one_speed_and_nearly_one(mirror, bmirror, tmp_path, n, want):
    """All vy equal: one bucket of the run's whole group pairs with h = 0, the members left over in the remainder; the same
    cut for speeds spread over less than the cap (r / 8 = 0.0375 wide)."""
    rng = np.random.default_rng(n)
    for vy in (same(0.37), same(-0.37), spread(0.30, 0.33, rng)):
        sph = pool([(0.5, n, vy)], rng)
        lay = check_layout(mirror, bmirror, tmp_path, sph)
        assert bucket_sizes(lay) == [want], (n, bucket_sizes(lay))
        r = lay["runs"][0]
        assert len(r["order"]) - r["bucketed"] == n - want[0]
    b = lay["runs"][0]["buckets"][0]
    assert 0.30 < np.uint32(b["v0_bits"]).view(f32) < 0.33


def test_no_bucket_forms_over_a_wide_spread(mirror, bmirror, tmp_path):
    rng = np.random.default_rng(1)
    sph = pool([(0.5, 200, spread(0.1, 0.5, rng)), (1.5, 64, spread(-0.5, 0.5, rng))], rng)
    lay = check_layout(mirror, bmirror, tmp_path, sph)
    assert bucket_sizes(lay) == [[], []]
    assert [r["order"] for r in lay["runs"]] == [r["members"] for r in lay["runs"]]  # the parent's slot order


def test_negative_and_mixed_sign_speeds(mirror, bmirror, tmp_path):
    rng = np.random.default_rng(2)
    mixed = lambda n: np.where(np.arange(n) % 2 == 0, rng.uniform(-0.21, -0.19, n), rng.uniform(0.19, 0.21, n))  # noqa: E731
    around_zero = lambda n: rng.choice([-1.0, 1.0], n) * rng.uniform(1e-6, 0.015, n)  # noqa: E731  (one bucket across the sign)
    sph = pool([(0.5, 160, mixed), (1.5, 80, spread(-0.45, -0.43, rng)), (2.5, 96, around_zero)], rng)
    lay = check_layout(mirror, bmirror, tmp_path, sph)
    assert bucket_sizes(lay) == [[80, 80], [80], [96]]
    v0 = [np.uint32(b["v0_bits"]).view(f32) for r in lay["runs"] for b in r["buckets"]]
    assert v0[0] < 0 < v0[1] and v0[2] < 0 and abs(v0[3]) < 0.015


def test_two_runs_many_buckets_and_a_remainder(mirror, bmirror, tmp_path):
    """A run dense enough for several buckets (mixed radii: the cap follows the smallest), one too sparse for any."""
    rng = np.random.default_rng(3)
    sph = pool([(0.2, 3000, spread(0.1, 0.5, rng)), (1.1, 300, spread(0.1, 0.5, rng))], rng, r=(0.15, 0.3))
    lay = check_layout(mirror, bmirror, tmp_path, sph)
    sizes = bucket_sizes(lay)
    assert len(sizes[0]) >= 8 and sum(sizes[0]) >= 2700 and len(sizes[1]) <= 1, sizes


def test_heights_at_3e4_and_non_finite_speeds(mirror, bmirror, tmp_path):
    rng = np.random.default_rng(4)
    sph = pool([(0.5, 100, spread(0.2, 0.22, rng))], rng, y0=3.0e4)
    bad = np.flatnonzero((sph[:, 4] >= 0.2) & (sph[:, 4] <= 0.22))[:3]
    sph[bad, 4] = [np.inf, -np.inf, np.nan]  # stay out of every bucket
    lay = check_layout(mirror, bmirror, tmp_path, sph)
    assert bucket_sizes(lay) == [[96]]
    r = lay["runs"][0]
    assert set(bad.tolist()) <= set(r["order"][r["bucketed"]:])


# ---- conservativeness ------------------------------------------------------------------------------------------------------
def aimed_rays(sph, rng, n):
    """Rays against a pool: each aimed at a point at distance u·r of one sphere's centre at the ray's time — u within 1e-3 of
    the rim for half of them (grazing), the rest anywhere up to 1.3 r; times 0, 1 and random; a third of the rays horizontal at
    the target's height (|e2y| = 1 up to rounding), a third nearly so."""
    k = rng.integers(0, len(sph), n)
    time = np.select([np.arange(n) % 3 == 0, np.arange(n) % 3 == 1], [0.0, 1.0], rng.random(n))
    u = np.where(rng.random(n) < 0.5, 1.0 + rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-7, -3, n), rng.uniform(0, 1.3, n))
    off = rng.normal(size=(n, 3))
    off /= np.linalg.norm(off, axis=1, keepdims=True)
    tgt = sph[k, 0:3] + sph[k, 3:6] * time[:, None] + off * (sph[k, 6] * u)[:, None]
    o = tgt + rng.normal(size=(n, 3)) * [12.0, 3.0, 12.0]
    kind = rng.integers(0, 3, n)
    o[kind == 0, 1] = tgt[kind == 0, 1]
    o[kind == 1, 1] = tgt[kind == 1, 1] + rng.uniform(-1e-4, 1e-4, (kind == 1).sum())
    d = (tgt - o) * rng.uniform(0.3, 3.0, (n, 1))
    # (the aim is off the rim by the rounding of o and d: both sides of it are hit)
    return np.concatenate([o, d, time[:, None]], 1)


def test_bucket_form_is_conservative(bmirror, tmp_path):
    rng = np.random.default_rng(11)
    for y0 in (0.0, 3.0e4):
        sph = pool([(0.2, 400, spread(0.2, 0.26, rng)), (1.0, 160, spread(-0.31, -0.30, rng))], rng, r=(0.15, 0.3), y0=y0)
        rays = aimed_rays(sph[(sph[:, 4] != 0)], rng, 4000)
        S = max(np.max(np.linalg.norm(sph[:, 0:3], axis=1) + np.abs(sph[:, 4]) + sph[:, 6]), np.max(np.linalg.norm(rays[:, 0:3], axis=1))) * (1 + 1e-3)
        sp, rp = _write(tmp_path, "s.bin", sph), _write(tmp_path, "r.bin", rays)
        assert sum(map(len, bucket_sizes(_run(bmirror, tmp_path, "layout", sp)))) >= 3
        for f64_rays in (0, 1):
            au = _run(bmirror, tmp_path, "audit", sp, rp, repr(S), f64_rays)
            print("bucket-form audit", y0, "f64 rays" if f64_rays else "f32 rays", au)
            assert au["pairs"] > 1.5e6 and au["f64_hits"] > 2000, au
            assert au["false_negatives"] == 0 and au["pad_passes"] == 0, au


def test_bucket_form_is_conservative_on_grazing_rays_and_big_coordinates(bmirror, tmp_path):
    """kat_records' adversarial (ray, sphere) pairs, each sphere in a bucket whose speed is the whole r / 16 off its own."""
    import kat_records as K

    rng = np.random.default_rng(9)
    for shift in (0.0, 3.0e4):
        rec = K.random_sphere_hits(rng, 40_000, big=True)
        rec[:, 0:3] = K.f32r(rec[:, 0:3] + shift)
        rec[:, 7:10] = K.f32r(rec[:, 7:10] + shift)
        rec = rec[(rec[:, 3] == 0) & (rec[:, 5] == 0)]
        sph, rays = rec[:, 0:7], rec[:, 7:14]
        S = max(np.max(np.linalg.norm(sph[:, 0:3], axis=1) + np.linalg.norm(sph[:, 3:6], axis=1) + sph[:, 6]),
                np.max(np.linalg.norm(rays[:, 0:3], axis=1))) * (1 + 1e-3)
        for f64_rays in (0, 1):
            au = _run(bmirror, tmp_path, "pairs", _write(tmp_path, "s.bin", sph), _write(tmp_path, "r.bin", rays), repr(S), f64_rays)
            assert au["pairs"] == len(rec) and au["f64_hits"] > 10_000, (shift, au)
            assert au["false_negatives"] == 0 and au["pad_passes"] == 0, (shift, f64_rays, au)


def test_bucket_form_tightness_over_config3_segments(bmirror, tmp_path):
    """Config 3's y-moving run (8,025 members): all but the few dozen of its highest speeds are in buckets, and over the segments
    test_plane_form_has_no_false_negatives_over_config3_segments uses, the bucket form passes at most (1 + 1/16)² times what the
    parent's form passes, + that test's slack of 1000.  Measured (f32 rays / f64 rays): DESIGN.md §6."""
    sph, rays, S = _config3_segments(np.random.default_rng(5))
    sp, rp = _write(tmp_path, "s.bin", sph), _write(tmp_path, "r.bin", rays)
    lay = _run(bmirror, tmp_path, "layout", sp)
    sizes = bucket_sizes(lay)
    print("config 3 buckets:", sizes)
    assert len(sizes) == 1 and sum(sizes[0]) >= 7900 and len(sizes[0]) >= 10
    for f64_rays in (0, 1):
        au = _run(bmirror, tmp_path, "audit", sp, rp, repr(S), f64_rays)
        print("bucket-form tightness", "f64 rays" if f64_rays else "f32 rays", au)
        assert au["pairs"] == len(rays) * sum(sizes[0]) and au["f64_hits"] > 8000, au
        assert au["false_negatives"] == 0 and au["pad_passes"] == 0, au
        assert au["f64_hits"] <= au["candidates"], au
        assert au["candidates"] <= (1 + 1 / CAP) ** 2 * au["parent_candidates"] + 1000, au


# ---- ISA -------------------------------------------------------------------------------------------------------------------
def test_bucket_loop_issues_six_packed_fmas_per_sphere_pair(tmp_path):
    from rayz_amd import _build

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    asm = tmp_path / "dev.s"
    flags = [f for f in _build.HIPFLAGS if f not in ("-fPIC", "-Wall", "-Wextra")]
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-o", str(asm), os.path.join(ROOT, "rayz_amd", "csrc", "rayz_hip.hip")],
                   check=True, capture_output=True, timeout=600)
    text = asm.read_text()
    for name in ("_ZN8rayz_dev12trace_kernelIfLi1EEEvNS_9TraceArgsIT_EE", "_ZN8rayz_dev20adaptive_pass_kernelIfLi1EEEvNS_9TraceArgsIT_EE"):
        body = text[text.index(name + ":"):]
        body = [l for l in body[:body.index(".Lfunc_end")].split("\n") if l.strip() and not l.strip().startswith(";")]
        labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\w+):", l)] if m}
        per_pair = []
        for i, l in enumerate(body):  # the scan loops, found as tests/test_plane_runs.py finds them
            m = re.search(r"s_cbranch_\w+ (\.LBB\w+)", l)
            if m and labels.get(m.group(1), i) < i and i - labels[m.group(1)] < 100:
                loop = body[labels[m.group(1)]:i + 1]
                pk = sum("v_pk_fma_f32" in x for x in loop)
                if pk > 1:
                    assert not any("v_readlane" in x or "scratch_" in x for x in loop), "a spilled register is read in a scan loop"
                    per_pair.append(pk)
        # static plane, static loose, mov-Y plane, mov-Y loose, then the buckets: the static plane form once more
        assert per_pair == [2 * 6 * G // 2, 2 * 7 * G // 2, 2 * 7 * G // 2, 2 * 8 * G // 2, 2 * 6 * G // 2], (name, per_pair)
