"""One-radius sets of the flat list's static plane runs and speed buckets: members whose |radius| + h lie
within r_min / 16 of each other are tested with ONE padded r², the set's, in blocks of cx and cz alone.  CPU checks, through a C++
mirror built here (tests/one_radius_mirror.cpp, which compiles the library's own rayz_amd/csrc/plane_runs.hpp):
  * layout over random pools: every set holds whole iterations of the set loop and at least 64 members, lies at the front of its
    run or bucket, is ordered by (|radius| + h, pool index) and obeys the cap; what no set took keeps the order it had; the runs
    and buckets themselves (first, end, members, v0) are what the parent's layout made; leftovers of a bucket are whole group pairs;
  * the set form in f32 exactly as the kernel evaluates it (xy basis) passes every (ray, member, time) pair whose f64 discriminant
    is >= 0, never fewer pairs than the XY form the member had; the set's R2 (the library's own class_set_r2, which the upload calls)
    is >= every member's own padded square and at most (1 + 1/16) times its radius beyond it (plus the spread of the set's pads):
    random rays at times in [0, 1], radii at both edges of the cap, heights at 3e4, negative radii;
  * config 3: the sets it forms and the candidates they let through under both forms;
  * AUTO reports (and launches) the set form from 1,024 set slots on, XY below."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_plane_runs import _config3_segments, _run, _write, mirror  # noqa: F401  (mirror: a fixture)
from test_speed_buckets import bmirror  # noqa: F401  (a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
CAP = 16   # plane_runs.hpp: kBucketCap
ITER = 16  # plane_runs.hpp: kSetIter = two groups of kSetGroup = 8
f32 = np.float32


@pytest.fixture(scope="module")
def omirror(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("one_radius") / "one_radius_mirror")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "one_radius_mirror.cpp")],
                   check=True, capture_output=True, timeout=300)
    return exe


def bucket_h(vy, v0):
    """plane_runs.hpp: bucket_h."""
    v0 = np.float64(v0)
    return np.maximum(np.abs(vy - v0), np.abs(np.float64(f32(vy)) - v0)) * (1.0 + 2.0 ** -50) + 1e-300


def pool(spec, rng, y0=0.0):
    """Sphere rows for [(cy, members, vy sampler or None for static, radius sampler), ...], 12 loose spheres beside them, shuffled."""
    rows = []
    for cy, n, vy, rad in spec:
        s = np.zeros((n, 7))
        s[:, 0], s[:, 1], s[:, 2], s[:, 6] = rng.uniform(-9, 9, n), y0 + cy, rng.uniform(-9, 9, n), rad(n)
        if vy is not None:
            s[:, 4] = vy(n)
        rows.append(s)
    extra = np.zeros((12, 7))
    extra[:, 0], extra[:, 1], extra[:, 2], extra[:, 6] = rng.uniform(-9, 9, 12), y0 + rng.uniform(-3, 3, 12), rng.uniform(-9, 9, 12), 0.3
    extra[6:, 4] = rng.uniform(0.1, 0.5, 6)
    sph = np.concatenate(rows + [extra])
    return sph[rng.permutation(len(sph))]


def check_layout(mirror, bmirror, omirror, tmp_path, sph):
    """The properties every set layout has; returns the mirror's layout."""
    sp = _write(tmp_path, "s.bin", sph)
    lay = _run(omirror, tmp_path, "layout", sp)
    assert lay["iter"] == ITER
    parent = _run(mirror, tmp_path, "layout", sp)["classes"]
    pb = _run(bmirror, tmp_path, "layout", sp)
    rad = np.abs(sph[:, 6])
    for c, cl in enumerate(lay["classes"]):
        # the runs (and the mov-Y class's buckets) are the parent's: the head, the run table and the bucket table do not change
        assert cl["plane_slots"] == parent[c]["plane_slots"] and len(cl["runs"]) == len(parent[c]["runs"])
        for j, (r, p) in enumerate(zip(cl["runs"], parent[c]["runs"])):
            assert (r["first"], r["end"], sorted(r["order"])) == (p["first"], p["end"], p["members"])
            if c == 1:
                q = pb["runs"][j]
                assert r["parent_order"] == q["order"]
                assert [(b["first"], b["end"], b["v0_bits"]) for b in r["buckets"]] == [(b["first"], b["end"], b["v0_bits"]) for b in q["buckets"]]
            else:
                assert r["parent_order"] == p["members"]
        # the parts sets are cut from: a static run's members, a bucket's
        parts = []
        for j, r in enumerate(cl["runs"]):
            if c == 0:
                parts.append((j, -1, r["first"], r["first"] + len(r["order"]), r["old_first"], 0.0))
            else:
                for b in r["buckets"]:
                    parts.append((j, len(parts), b["first"], b["end"], b["old_first"], float(np.uint32(b["v0_bits"]).view(f32))))
                rem = r["first"] + sum(b["end"] - b["first"] for b in r["buckets"])
                assert r["old_first"] == rem  # a y-moving run's 4-field remainder: where the bucket header has it
        seen = 0
        for j, b, first, end, old_first, v0 in parts:
            r = cl["runs"][j]
            order = r["order"][first - r["first"]:end - r["first"]]
            was = r["parent_order"][first - r["first"]:end - r["first"]]
            assert sorted(order) == sorted(was)  # every member of the part in exactly one place of it
            sets = [t for t in cl["sets"] if t["run"] == j and t["bucket"] == b]
            assert cl["sets"][seen:seen + len(sets)] == sets  # the table: run by run, part by part
            seen += len(sets)
            at = first
            for t in sets:
                n = t["end"] - t["first"]
                assert t["first"] == at and n % ITER == 0 and n >= 64, t  # whole iterations, back to back from the part's first slot
                m = np.array(order[at - first:at - first + n])
                key = rad[m] + (bucket_h(sph[m, 4], v0) if c == 1 else 0.0)
                assert list(zip(key.tolist(), m.tolist())) == sorted(zip(key.tolist(), m.tolist()))
                assert t["Rp"] == key.max() and key.max() - key.min() <= rad[m].min() / CAP, (t, key.min(), key.max())
                assert np.uint32(t["v0_bits"]).view(f32) == f32(v0)
                at = t["end"]
            assert at == old_first <= end
            left = order[at - first:]
            assert left == [m for m in was if m in set(left)]  # what no set took keeps its old order
            if c == 1:
                assert (end - old_first) % 8 == 0  # a bucket's leftovers: whole group pairs of its 3-field loop
        assert seen == len(cl["sets"])
    return lay


def set_sizes(lay):
    return [[t["end"] - t["first"] for t in cl["sets"]] for cl in lay["classes"]]


def same(v):
    return lambda n: np.full(n, v)


@pytest.mark.parametrize("n, want", [(63, []), (64, [64]), (71, [64]), (72, [64]), (73, [64]), (80, [80]), (200, [192])])
def test_one_radius_runs_and_buckets(mirror, bmirror, omirror, tmp_path, n, want):
    """All radii equal: a static run's whole iterations form one set; so do a bucket's (the bucket itself is whole group pairs)."""
    rng = np.random.default_rng(n)
    lay = check_layout(mirror, bmirror, omirror, tmp_path, pool([(0.5, n, None, same(0.3)), (1.5, n, same(0.37), same(-0.25))], rng))
    nb = n // 8 * 8
    assert set_sizes(lay) == [want, [nb // ITER * ITER] if nb >= 64 else []], set_sizes(lay)
    if want:
        r = lay["classes"][0]["runs"][0]
        assert r["old_first"] - r["first"] == want[0] and len(r["order"]) == n


def test_radii_inside_and_outside_the_cap(mirror, bmirror, omirror, tmp_path):
    """Radii 0.32 .. 0.34 (one set: 0.02 = 0.32 / 16), then 0.3401 .. (a second set), then radii all apart (left over)."""
    rng = np.random.default_rng(3)
    rad = np.concatenate([np.linspace(0.32, 0.34, 70), np.linspace(0.3401, 0.36, 66), 0.5 * 1.2 ** np.arange(9)])
    lay = check_layout(mirror, bmirror, omirror, tmp_path, pool([(0.5, len(rad), None, lambda n: rng.permutation(rad))], rng))
    assert set_sizes(lay) == [[64, 64], []], set_sizes(lay)
    r = lay["classes"][0]["runs"][0]
    assert len(r["order"]) - (r["old_first"] - r["first"]) == len(rad) - 128
    # one step over the cap splits: 65 members at 0.32 and 65 at 0.32 · (1 + 1/16) + 1e-9
    rad = np.concatenate([np.full(65, 0.32), np.full(65, 0.32 * (1 + 1 / 16) + 1e-9)])
    lay = check_layout(mirror, bmirror, omirror, tmp_path, pool([(0.5, 130, None, lambda n: rng.permutation(rad))], rng))
    assert set_sizes(lay) == [[64, 64], []]
    rad = np.concatenate([np.full(65, 0.32), np.full(65, 0.32 * (1 + 1 / 16) - 1e-9)])
    lay = check_layout(mirror, bmirror, omirror, tmp_path, pool([(0.5, 130, None, lambda n: rng.permutation(rad))], rng))
    assert set_sizes(lay) == [[128], []]


def test_no_set_forms_where_every_radius_differs(mirror, bmirror, omirror, tmp_path):
    rng = np.random.default_rng(4)
    lay = check_layout(mirror, bmirror, omirror, tmp_path,
                       pool([(0.5, 100, None, lambda n: 0.05 * 1.07 ** np.arange(n)), (1.0, 100, same(0.2), lambda n: 0.05 * 1.07 ** np.arange(n))], rng))
    assert set_sizes(lay) == [[], []]
    for cl in lay["classes"]:
        for r in cl["runs"]:
            assert r["order"] == r["parent_order"]  # nothing moves: the parent's slots


def test_two_radius_classes_in_one_bucket_and_random_pools(mirror, bmirror, omirror, tmp_path):
    rng = np.random.default_rng(5)
    two = lambda n: rng.permutation(np.concatenate([np.full(n // 2, 0.2), np.full(n - n // 2, -0.4)]))  # noqa: E731
    lay = check_layout(mirror, bmirror, omirror, tmp_path, pool([(0.7, 200, lambda n: rng.uniform(0.300, 0.305, n), two)], rng))
    assert set_sizes(lay) == [[], [96, 96]], set_sizes(lay)
    formed = 0
    for seed in range(12):
        rng = np.random.default_rng(100 + seed)
        spec = []
        for k in range(int(rng.integers(1, 5))):
            n = int(rng.integers(60, 260))
            classes = rng.choice([0.2, 0.21, 0.3, -0.3, 0.45], int(rng.integers(1, 4)))
            rad = lambda n, classes=classes: rng.choice(classes, n) * np.where(rng.random(n) < 0.2, rng.uniform(0.5, 2.0, n), 1.0)  # noqa: E731
            vy = None if rng.random() < 0.5 else (lambda n: rng.choice([0.2, -0.4], n) + rng.uniform(-0.01, 0.01, n))
            spec.append((0.5 * k, n, vy, rad))
        lay = check_layout(mirror, bmirror, omirror, tmp_path, pool(spec, rng, y0=3.0e4 if seed % 4 == 3 else 0.0))
        formed += sum(map(len, set_sizes(lay)))
    assert formed >= 12, formed


def _audit(omirror, tmp_path, sph, rays, S):
    sp, rp = _write(tmp_path, "s.bin", sph), _write(tmp_path, "r.bin", rays)
    out = []
    for f64_rays in (0, 1):
        au = _run(omirror, tmp_path, "audit", sp, rp, repr(S), f64_rays)
        print(au)
        assert au["false_negatives"] == 0 and au["lost"] == 0, au  # conservative, and a superset of the XY form's candidates
        assert au["candidates"] >= au["xy_candidates"] >= au["f64_hits"], au
        # R2 >= every member's own padded square (the XY form's r², or its bucket's r2b): what makes the set form a superset
        assert au["min_r2_over_own"] >= 1.0, au
        # a member as the sphere of radius R' is at most (1 + 1/16) of its own |radius| + h: the two pads differ by 40u·(R' − |r| − h)
        # and each square by one f32 rounding ..
        assert au["max_member_ratio"] <= (1 + 1 / CAP) * (1 + 1e-6), au
        # .. and the set's R2 is its LARGEST member's, so a member carries at most the spread of its set's pads more
        assert au["max_radius_ratio"] <= (1 + 1 / CAP) * (1 + 1e-6) + au["max_pad_spread"], au
        out.append(au)
    return out


def _rays_at(rng, sph, n):
    """Random rays aimed at members of the pool where they are at the ray's time: through them, at their rims, just past them."""
    k = rng.integers(0, len(sph), n)
    t = rng.random(n)
    t[: n // 8], t[n // 8: n // 4] = 0.0, 1.0
    c = sph[k, 0:3] + sph[k, 3:6] * t[:, None]
    o = c + rng.normal(size=(n, 3)) * rng.uniform(1.0, 30.0, (n, 1))
    off = rng.normal(size=(n, 3))
    off /= np.linalg.norm(off, axis=1, keepdims=True)
    off *= (np.abs(sph[k, 6]) * np.where(rng.random(n) < 0.5, 1.0 + rng.uniform(-1e-4, 1e-4, n), rng.uniform(0, 1.5, n)))[:, None]
    d = (c + off - o) * rng.uniform(0.3, 3.0, (n, 1))
    return np.concatenate([o, d, t[:, None]], 1)


@pytest.mark.parametrize("y0", [0.0, 3.0e4])
def test_set_form_has_no_false_negatives(omirror, tmp_path, y0):
    """Radii at both edges of the cap inside one set, negative radii, a bucket whose speeds fill its whole width."""
    rng = np.random.default_rng(7)
    hi = 0.32 + 0.32 / CAP * (1 - 1e-9)  # the largest radius a set of 0.32s takes
    edge = lambda n: rng.permutation(np.where(np.arange(n) % 2 == 0, 0.32, hi)) * rng.choice([-1.0, 1.0], n)  # noqa: E731
    sph = pool([(0.5, 130, None, edge), (1.1, 130, lambda n: 0.3 + rng.uniform(-0.005, 0.005, n), edge),
                (1.9, 70, None, same(-0.25))], rng, y0=y0)
    rays = _rays_at(rng, sph, 3000)
    S = max(np.max(np.linalg.norm(sph[:, 0:3], axis=1) + np.abs(sph[:, 4]) + np.abs(sph[:, 6])) * (1 + 1e-3), np.max(np.linalg.norm(rays[:, 0:3], axis=1)))
    for au in _audit(omirror, tmp_path, sph, rays, S):
        assert au["pairs"] >= 3000 * (128 + 64 + 64) and au["f64_hits"] > 1000, au  # the static runs' sets, and at least one in the bucket
        assert y0 != 0.0 or au["max_radius_ratio"] > 1.06, au  # the static set spans the whole cap (at 3e4 the pad outweighs it)
        assert au["min_r2_over_own"] < 1.001, au  # .. and its largest members sit just under R2: a smaller R2 would fail above


def test_config3_sets_and_their_candidates(omirror, tmp_path):
    """Config 3: the static run and every bucket of radius-0.2 spheres become sets; what the larger radius lets through."""
    sph, rays, S = _config3_segments(np.random.default_rng(5), n_primary=1000, n_bounce=3000)
    lay = _run(omirror, tmp_path, "layout", _write(tmp_path, "s.bin", sph))
    in_sets = sum(t["end"] - t["first"] for cl in lay["classes"] for t in cl["sets"])
    in_runs = sum(len(r["order"]) for cl in lay["classes"] for r in cl["runs"])
    print("config 3:", in_sets, "of", in_runs, "run members in", sum(len(cl["sets"]) for cl in lay["classes"]), "sets")
    # every grid sphere has radius 0.2: each static run and each bucket is one set of its whole iterations
    parts = [len(r["order"]) for r in lay["classes"][0]["runs"]] + [b["end"] - b["first"] for r in lay["classes"][1]["runs"] for b in r["buckets"]]
    assert sorted(t["end"] - t["first"] for cl in lay["classes"] for t in cl["sets"]) == sorted(n // ITER * ITER for n in parts if n // ITER * ITER >= 64)
    for au in _audit(omirror, tmp_path, sph, rays, S):
        assert au["candidates"] <= (1 + 1 / CAP) ** 2 * au["xy_candidates"] + 1000, au


@pytest.mark.parametrize("n, form", [(1024, 3), (1023, 2), (100, 2)])
def test_auto_reports_the_set_form_from_1024_set_slots(n, form):
    """plane_runs.hpp: kSetPayoffSlots, through rayz_hip_scene_get_scan_form (host only): a static run of n spheres of one radius puts
    n // 16 * 16 of them in a set; AUTO takes ONE_RADIUS (3) from 1,024 set slots on and XY (2) below; a form that was set is reported."""
    from rayz_amd import capi, render
    from test_plane_runs_gpu import Scene

    s = Scene(70 + n % 2, width=32)
    for _ in range(n):
        s.sphere((s.rng.uniform(-12, 12), 0.3, s.rng.uniform(-12, 12)), 0.12)
    ds = render.DeviceScene(s.loose().build(spp=4, bounces=4).scene_desc())
    try:
        assert ds.scan_form == form
        for forced in (capi.SCAN_FORM_XZ, capi.SCAN_FORM_XY, capi.SCAN_FORM_ONE_RADIUS):
            ds.scan_form = forced
            assert ds.scan_form == forced
        ds.scan_form = capi.SCAN_FORM_AUTO
        assert ds.scan_form == form
    finally:
        ds.close()
