"""Primary lists: the beam test `may_hit` of rayz_amd/csrc/primary_lists.hpp, compiled into a stand-alone host
program (tests/primary_lists_mirror.cpp), against the exact f64 quadratic.  Per scene of tests/primary_lists_scenes.py at least
20,000 samples (pixel, lens point of the SQUARE [-1, 1]², jitter in [-½, ½]², time in [0, 1]; a quarter of them at the extreme
corners: lens ±1, jitter ±½, time 0 or 1); the mirror decides every (sample, sphere) pair — a root at t > 0 — and every hit must be
in the pixel's list unless the pixel has none; once for the f64 camera's rays and once (`check32`) for the rays the f32 kernels
trace, formed in float from the camera narrowed to float as camera_ray<float> forms them.  Zero misses.  The test does not hide behind the fallback: at most 10 % of a
scene's pixels may be without a list, except in the scene built to overflow, where every pixel of a stated rectangle must be.

Mutations of the header, each run once against this file and each failing it (not committed): the sweep taken at time 0 only
(v dropped from beam_may_hit) — all 7 scenes fail; the lens bound dropped (lens = 0 in pixel_beam) — lens_disc_cuts_a_sphere fails
(the other lenses are narrower than the pixel beam where their spheres are); the pixel half width dropped (0.5·(|du| + |dv|) → 0) —
all 7 fail.  A fourth, kF32 = kJitter = 0 (the margins for the f32 kernels' roundings), was run too and does NOT fail this file, not
even on a camera with parallel pixel steps (where ½(|du| + |dv|) is attained) over spheres of radius 0.03 at 3·10⁴: the derivation's own
slack — the corners' triangle inequality, the factor L / (L − A − B) on the far half width — exceeds an f32 rounding at that
magnitude.  Those two margins rest on §4.19's step 2, not on a test."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import primary_lists_scenes as S
from test_plane_runs import _spheres, _write

HERE = os.path.dirname(os.path.abspath(__file__))
N_SAMPLES = 24_000


@pytest.fixture(scope="module")
def pmirror(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("primary_lists") / "primary_lists_mirror")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "primary_lists_mirror.cpp")],
                   check=True, capture_output=True, timeout=300)
    return exe


def samples(rng, n):
    """(n, 7): px, py, lens x, lens y, jitter x, jitter y, time; the last quarter at extreme corners."""
    s = np.empty((n, 7))
    s[:, 0], s[:, 1] = rng.integers(0, S.W, n), rng.integers(0, S.H, n)
    s[:, 2:4] = rng.uniform(-1.0, 1.0, (n, 2))
    s[:, 4:6] = rng.uniform(-0.5, 0.5, (n, 2))
    s[:, 6] = rng.uniform(0.0, 1.0, n)
    q = n - n // 4
    s[q:, 2:4] = rng.choice([-1.0, 1.0], (n - q, 2))
    s[q:, 4:6] = rng.choice([-0.5, 0.5], (n - q, 2))
    s[q:, 6] = rng.choice([0.0, 1.0], n - q)
    return s


def list_counts(pmirror, tmp_path, t):
    sp, cp = _write(tmp_path, "s.bin", _spheres(t)), _write(tmp_path, "c.bin", S.camera_row(t.camera_desc()))
    r = subprocess.run([pmirror, "counts", str(sp), str(cp), str(S.W), str(S.H)], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return np.frombuffer(r.stdout, dtype=np.uint32).reshape(S.H, S.W), sp, cp


@pytest.mark.parametrize("name", S.NAMES)
def test_every_hit_of_a_pixels_camera_rays_is_in_its_list(pmirror, tmp_path, name):
    t = S.build(name)
    assert len(_spheres(t)) <= 300
    counts, sp, cp = list_counts(pmirror, tmp_path, t)
    no_list = counts == S.NO_LIST
    assert (counts[~no_list] <= S.K).all()
    if name == "overflow":
        x0, x1, y0, y1 = S.OVERFLOW_RECT
        assert no_list[y0:y1, x0:x1].all(), counts[y0:y1, x0:x1]
        assert 0 < no_list.sum() < 0.5 * no_list.size  # .. and lanes with and without lists share waves
    else:
        assert no_list.mean() <= 0.10, (name, no_list.mean())
    smp = _write(tmp_path, "smp.bin", samples(np.random.default_rng(7), N_SAMPLES))
    for mode in ("check", "check32"):  # the f64 camera's rays, and the rays the f32 kernels form from the camera narrowed to float
        r = subprocess.run([pmirror, mode, str(sp), str(cp), str(smp)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        got = json.loads(r.stdout)
        print(name, mode, got, "pixels without a list:", int(no_list.sum()), "mean list:", float(counts[~no_list].mean()), "max:", int(counts[~no_list].max()))
        assert got["samples"] == N_SAMPLES >= 20_000
        assert got["misses"] == 0, (mode, got)
        assert got["listed_hits"] >= 5_000, (mode, got)  # the lists, not the fallback, answered: a hit in a list for a quarter of the samples at least


def test_every_list_of_the_all_sky_scene_is_empty(pmirror, tmp_path):
    """What tests/test_primary_lists_gpu.py's all-sky frame rests on: every pixel has a list and it is empty."""
    counts, _, _ = list_counts(pmirror, tmp_path, S.build("all_sky"))
    assert (counts == 0).all(), counts
