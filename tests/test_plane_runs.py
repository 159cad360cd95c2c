"""Plane runs of the flat list's scan: the static and mov-Y spheres that share one f32 centre height are
scanned with cy·e2y + k2 hoisted out of the reject test.  CPU checks, through a C++ mirror built here
(tests/plane_filter_mirror.cpp, which compiles the library's own rayz_amd/csrc/plane_runs.hpp):
  * the run layout partitions every class, runs share one f32 cy and are padded to whole group pairs;
  * the plane form of the f32 test, with the scan's padded r², lets through every pair whose f64 discriminant is >= 0
    (config-3 segments and the adversarial records of kat_records, also shifted by 3e4; f32 rays and f64 rays narrowed);
  * pad slots never pass;
and an ISA check of the compiled f32 flat kernel: 6·G/2 packed FMAs per static plane group, 7·G/2 per mov-Y one."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from rayz_amd import capi, tracer

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
G = 4  # spheres per scan group (device_types.hpp: RAYZ_GROUP)


@pytest.fixture(scope="module")
def mirror(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("plane") / "plane_filter_mirror")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "plane_filter_mirror.cpp")],
                   check=True, capture_output=True, timeout=300)
    return exe


def _spheres(t):
    sd = t.scene_desc()
    raw = np.ctypeslib.as_array(C.cast(sd.spheres, C.POINTER(C.c_double)), shape=(sd.n_spheres * 8,)).reshape(-1, 8)
    return raw[:, :7].copy()  # cx cy cz vx vy vz r (the 8th double is material + pad)


def _run(mirror, tmp_path, *args):
    r = subprocess.run([mirror, *map(str, args)], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def _write(tmp_path, name, a):
    p = tmp_path / name
    np.ascontiguousarray(a, dtype=np.float64).tofile(p)
    return p


def test_run_layout_partitions_every_class(mirror, tmp_path):
    for t in (tracer.randomBouncing(64, -50, 50, seed=42), tracer.randomBouncing(64, seed=42),
              tracer.randomBouncing(64, -5, 5, seed=42), tracer.threeSpheres(64, seed=1)):
        sph = _spheres(t)
        lay = _run(mirror, tmp_path, "layout", _write(tmp_path, "s.bin", sph))
        static = (sph[:, 3:6] == 0).all(1)
        movy = (sph[:, 3] == 0) & (sph[:, 5] == 0) & (sph[:, 4] != 0)
        for c, want in enumerate((np.flatnonzero(static), np.flatnonzero(movy))):
            cl = lay["classes"][c]
            got = [m for r in cl["runs"] for m in r["members"]] + cl["loose"]
            assert sorted(got) == want.tolist()  # every sphere of the class in exactly one place
            at = 0
            cys = []
            for r in cl["runs"]:
                assert r["first"] == at and (r["end"] - r["first"]) % (2 * G) == 0
                assert len(r["members"]) >= 64 and r["end"] - r["first"] - len(r["members"]) < 2 * G
                cy = np.float32(sph[r["members"], 1])
                assert (cy == np.float32(r["cy"])).all()  # one f32 height per run
                assert r["members"] == sorted(r["members"])  # pool order
                cys.append(r["cy"])
                at = r["end"]
            assert cl["plane_slots"] == at and cys == sorted(cys) and len(cys) <= 4
            assert not (np.isin(np.float32(sph[cl["loose"], 1]), np.float32(cys))).any()
    # randomBouncing's grid is one plane: config 3 puts all but the three large spheres and the ground in two runs
    lay = _run(mirror, tmp_path, "layout", _write(tmp_path, "s.bin", _spheres(tracer.randomBouncing(64, -50, 50, seed=42))))
    assert [len(c["runs"]) for c in lay["classes"]] == [1, 1] and lay["classes"][0]["runs"][0]["cy"] == pytest.approx(0.2)
    assert len(lay["classes"][0]["loose"]) == 4 and lay["classes"][1]["loose"] == []


def _config3_segments(rng, n_primary=3000, n_bounce=9000):
    """Segments of configs[2]'s frame: primary camera rays, and rays leaving points on the scene's spheres (diffuse-like,
    mirror-like and grazing directions, origins on the r = 1000 ground included) at random times."""
    t = tracer.randomBouncing(1920, -50, 50, seed=42)
    sph = _spheres(t)
    rays = []
    for _ in range(n_primary):
        o, d = t.get_ray(int(rng.integers(0, 1920)), int(rng.integers(0, 1080)))
        rays.append(np.concatenate([o, d, [rng.random()]]))
    k = rng.integers(0, len(sph), n_bounce)
    k[: n_bounce // 4] = np.argmax(sph[:, 6])  # the ground
    time = rng.random(n_bounce)
    nrm = rng.normal(size=(n_bounce, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    nrm[: n_bounce // 4] = np.abs(nrm[: n_bounce // 4]) * [0.05, 1, 0.05] + [0, 0.2, 0]  # the ground's upper side
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    o = sph[k, 0:3] + sph[k, 3:6] * time[:, None] + nrm * sph[k, 6:7] * (1 + 1e-7)
    dirs = rng.normal(size=(n_bounce, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    graze = rng.random(n_bounce) < 0.3
    dirs[graze] -= nrm[graze] * (dirs[graze] * nrm[graze]).sum(1, keepdims=True) * 0.999  # nearly tangent
    dirs = np.where((dirs * nrm).sum(1, keepdims=True) < 0, -dirs, dirs) + nrm * 1e-3
    rays = np.concatenate([np.array(rays), np.concatenate([o, dirs * rng.uniform(0.5, 2, (n_bounce, 1)), time[:, None]], 1)])
    S = max(np.max(np.linalg.norm(sph[:, 0:3], axis=1) + np.linalg.norm(sph[:, 3:6], axis=1) + sph[:, 6]) * (1 + 1e-3),
            np.max(np.linalg.norm(rays[:, 0:3], axis=1)))
    return sph, rays, S


def test_plane_form_has_no_false_negatives_over_config3_segments(mirror, tmp_path):
    sph, rays, S = _config3_segments(np.random.default_rng(5))
    sp, rp = _write(tmp_path, "s.bin", sph), _write(tmp_path, "r.bin", rays)
    for f64_rays in (0, 1):
        au = _run(mirror, tmp_path, "audit", sp, rp, repr(S), f64_rays)
        assert au["pairs"] > 1.0e8 and au["f64_hits"] > 10_000, au
        assert au["false_negatives"] == 0, au
        assert au["pad_passes"] == 0, au
        assert au["f64_hits"] <= au["candidates"] <= 1.25 * au["f64_hits"] + 1000, au
        print("plane-form filter audit", "f64 rays" if f64_rays else "f32 rays", au)


def test_plane_form_has_no_false_negatives_on_grazing_rays_and_big_coordinates(mirror, tmp_path):
    """kat_records' adversarial (ray, sphere) pairs, each sphere its own run (its own cy), static and mov-Y ones."""
    import kat_records as K

    rng = np.random.default_rng(9)
    for shift in (0.0, 3.0e4):
        rec = K.random_sphere_hits(rng, 40_000, big=True)
        rec[:, 0:3] = K.f32r(rec[:, 0:3] + shift)
        rec[:, 7:10] = K.f32r(rec[:, 7:10] + shift)
        plane = (rec[:, 3] == 0) & (rec[:, 5] == 0)  # static or mov-Y: the classes that have plane runs
        rec = rec[plane]
        sph, rays = rec[:, 0:7], rec[:, 7:14]
        S = max(np.max(np.linalg.norm(sph[:, 0:3], axis=1) + np.linalg.norm(sph[:, 3:6], axis=1) + sph[:, 6]),
                np.max(np.linalg.norm(rays[:, 0:3], axis=1))) * (1 + 1e-3)
        for f64_rays in (0, 1):
            au = _run(mirror, tmp_path, "pairs", _write(tmp_path, "s.bin", sph), _write(tmp_path, "r.bin", rays), repr(S), f64_rays)
            assert au["pairs"] == len(rec) and au["f64_hits"] > 10_000, (shift, au)
            assert au["false_negatives"] == 0 and au["pad_passes"] == 0, (shift, f64_rays, au)


def test_plane_loops_issue_one_packed_fma_less_per_sphere_pair(tmp_path):
    from rayz_amd import _build

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    asm = tmp_path / "dev.s"
    flags = [f for f in _build.HIPFLAGS if f not in ("-fPIC", "-Wall", "-Wextra")]
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-o", str(asm), os.path.join(ROOT, "rayz_amd", "csrc", "rayz_hip.hip")],
                   check=True, capture_output=True, timeout=600)
    text = asm.read_text()
    name = "_ZN8rayz_dev12trace_kernelIfLi1EEEvNS_9TraceArgsIT_EE"
    body = text[text.index(name + ":"):]
    body = [l for l in body[:body.index(".Lfunc_end")].split("\n") if l.strip() and not l.strip().startswith(";")]
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\w+):", l)] if m}
    # the scan loops: the innermost backward branches whose body is packed FMAs (one iteration = one group pair = 2·G tests)
    per_pair = []
    for i, l in enumerate(body):
        m = re.search(r"s_cbranch_\w+ (\.LBB\w+)", l)
        if m and labels.get(m.group(1), i) < i and i - labels[m.group(1)] < 100:
            loop = body[labels[m.group(1)]:i + 1]
            pk = sum("v_pk_fma_f32" in x for x in loop)
            if pk:
                assert not any("v_readlane" in x or "scratch_" in x for x in loop), "a spilled register is read in a scan loop"
                per_pair.append(pk)
    # static plane, static loose, mov-Y plane, mov-Y loose (slot order); per group: 6·G/2, 7·G/2, 7·G/2, 8·G/2
    assert per_pair[:4] == [2 * 6 * G // 2, 2 * 7 * G // 2, 2 * 7 * G // 2, 2 * 8 * G // 2], per_pair


def _groups(spec, rng):
    """Sphere rows for [(class, cy, members), ...] (class 0 static, 1 mov-Y), shuffled into one pool order."""
    rows = []
    for cls, cy, n in spec:
        s = np.zeros((n, 7))
        s[:, 0], s[:, 1], s[:, 2], s[:, 6] = rng.uniform(-9, 9, n), cy, rng.uniform(-9, 9, n), 0.3
        s[:, 4] = rng.uniform(0.1, 0.5, n) * cls
        rows.append(s)
    sph = np.concatenate(rows)
    return sph[rng.permutation(len(sph))]


def test_run_layout_keeps_the_four_largest_groups(mirror, tmp_path):
    """More than four qualifying heights: the four largest groups become runs, a tie in size goes to the smaller cy BITS
    (+0 before a positive height before -0 before a negative one), the runs are laid out in ascending cy (+0 before -0),
    groups of 63 and the groups left over stay loose."""
    rng = np.random.default_rng(2)
    cases = [  # (class, [(cy, members)]), the runs wanted in layout order
        (0, [(1.5, 64), (-0.5, 64), (2.5, 90), (0.5, 80), (3.5, 70)], [(0.5, 80), (1.5, 64), (2.5, 90), (3.5, 70)]),
        (0, [(0.25, 100), (-2.0, 65), (0.75, 64), (1.25, 72), (3.0, 64), (4.0, 63), (-0.0, 65)],
         [(-2.0, 65), (-0.0, 65), (0.25, 100), (1.25, 72)]),
        (1, [(-0.0, 64), (0.0, 64), (5.0, 64), (-5.0, 64), (6.0, 64)], [(0.0, 64), (-0.0, 64), (5.0, 64), (6.0, 64)]),
    ]
    bits = lambda x: int(np.float32(x).view(np.uint32))  # noqa: E731
    for c, spec, want in cases:
        sph = _groups([(c, cy, n) for cy, n in spec], rng)
        cl = _run(mirror, tmp_path, "layout", _write(tmp_path, "s.bin", sph))["classes"][c]
        # (the run's height as its members hold it: the layout's JSON prints -0 as an integer)
        got = [(bits(sph[r["members"][0], 1]), len(r["members"])) for r in cl["runs"]]
        assert got == [(bits(cy), n) for cy, n in want], (spec, got)
        at = 0
        for r in cl["runs"]:
            assert r["first"] == at and r["end"] - r["first"] == -(-len(r["members"]) // (2 * G)) * 2 * G
            at = r["end"]
        assert len(cl["loose"]) == sum(n for _, n in spec) - sum(n for _, n in want)


def test_mirror_plane_form_is_conservative_on_plane_blocks(mirror, tmp_path, oracle):
    """The mirror's plane form (tests/test_plane_runs_gpu.py holds the device to it bit for bit), from the padded r² the
    oracle returns for the record, passes every sphere whose f64 discriminant (mode A) is >= 0; pad slots never pass."""
    import kat_records as K

    rec = K.random_plane_blocks(np.random.default_rng(21), 100_000)
    a = oracle.kat_a(capi.KAT_SCAN_DISCS, rec)[:, :4]
    for prec in (capi.PRECISION_F32, capi.PRECISION_F64):
        r = rec.copy()
        r[:, 28:32] = oracle.kat_b(capi.KAT_SCAN_DISCS, rec, prec)[:, 8:12]
        m = mirror_discs(mirror, tmp_path, r, prec)
        assert (m[:, :4][a >= 0] >= 0).all(), int((m[:, :4][a >= 0] < 0).sum())
        assert not (m[:, 4:] >= 0).any()
        assert 0.1 < (m[:, :4] >= 0).mean() < 0.6


def mirror_discs(mirror, tmp_path, rec, prec):
    """The mirror's `discs` command: (n, 8) f32 = the plane form of the record's four spheres, then a pad slot's value."""
    p = _write(tmp_path, "rec.bin", rec)
    r = subprocess.run([mirror, "discs", str(p), str(int(prec == capi.PRECISION_F64))], capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr
    return np.frombuffer(r.stdout, dtype=np.float32).reshape(-1, 8)
