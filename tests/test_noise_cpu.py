"""The noise estimate of progressive rendering without a GPU: the numpy restatement tests/noise_ref.py against
answers worked by hand, and the estimate's calibration measured on the CPU oracle."""
import math

import numpy as np
import pytest

import noise_ref
from noise_cases import CASES, CLAMP_CASE
from rayz_amd import capi, tracer


def same(a, b):
    """Equal as values, NaN equal to NaN."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_closed_forms(case, f64):
    _, sums, sizes, want = case
    Q, var, rel2, sm = noise_ref.estimate(sums, sizes, f64)
    assert same(Q[0], want["q"]), (Q, want["q"])
    assert same(var[0], want["var"]) and same(rel2[0], want["rel2"]), (var, rel2, want)
    assert sm["unconverged"] == want["unconverged"] and sm["pixels"] == 1
    assert sm["chunks_done"] == len(sizes) and sm["samples_done"] == sum(sizes)
    assert same(sm["max_rel2"], want["rel2"])  # (one pixel: the maximum is the pixel's; the NaN case surfaces a NaN)
    assert same(sm["mean_var"], want["var"] if math.isfinite(want["var"]) else 0.0)


def test_all_zero_pixel_is_divided_by_the_floor():
    """den = floor2 when the mean is below the floor: rel2 = var / mean_floor²."""
    sums = np.array([[[0.25, 0, 0]], [[0.0, 0, 0]]])  # sizes 1, 1: var = 0.25²/4 = 2^-6, mean 2^-3
    _, var, rel2, _ = noise_ref.estimate(sums, [1, 1], mean_floor=0.5)
    assert var[0] == 2.0 ** -6 and rel2[0] == 2.0 ** -6 / 0.25
    _, var, rel2, _ = noise_ref.estimate(sums, [1, 1], mean_floor=2.0 ** -4)  # above the floor: / |mean|² = 2^-6
    assert rel2[0] == 1.0


def test_a_tiny_negative_d_is_clamped():
    _, sums, sizes, want = CLAMP_CASE
    M, Q = noise_ref.fold(sums, sizes, f64=False)
    D = Q - (M * M) / 3.0
    assert (D < 0).all() and (np.abs(D) < 1e-8).all(), D  # rounding alone (acc rounds up in f32): three equal chunks have no spread
    _, var, rel2, sm = noise_ref.estimate(sums, sizes)
    assert var[0] == 0.0 and rel2[0] == 0.0 and sm["unconverged"] == 0


def test_threshold_is_inclusive_and_nan_counts_as_unconverged():
    sums = np.array([[[3.0, 0, 0]], [[1.0, 0, 0]]])  # var = 1, mean 2: rel2 = 0.25 = 0.5²
    _, _, rel2, sm = noise_ref.estimate(sums, [1, 1], rel_error=0.5)
    assert rel2[0] == 0.25 and sm["unconverged"] == 0
    _, _, _, sm = noise_ref.estimate(sums, [1, 1], rel_error=0.49)
    assert sm["unconverged"] == 1
    both = np.concatenate([sums, np.array([[[math.nan, 0, 0]], [[1.0, 0, 0]]])], axis=1)
    _, _, rel2, sm = noise_ref.estimate(both, [1, 1], rel_error=0.5)
    assert sm["unconverged"] == 1 and math.isnan(sm["max_rel2"]) and sm["mean_var"] == 0.5  # (finite var only, over 2 pixels)


def test_fold_is_sequential_in_the_precision():
    """acc adds in R in chunk order (f32: 2^24 + 1 + 1 stays 2^24), Q in f64 from the narrowed chunk sums."""
    sums = np.array([[[2.0 ** 24, 0.1, 0]], [[1.0, 0.1, 0]], [[1.0, 0.1, 0]]])
    M32, Q32 = noise_ref.fold(sums, [1, 1, 1], f64=False)
    M64, Q64 = noise_ref.fold(sums, [1, 1, 1], f64=True)
    assert M32[0, 0] == 2.0 ** 24 and M64[0, 0] == 2.0 ** 24 + 2
    assert Q32[0, 0] == Q64[0, 0] == 2.0 ** 48 + 2
    t = float(np.float32(0.1))
    assert Q32[0, 1] == (t * t + t * t) + t * t and Q64[0, 1] == (0.1 * 0.1 + 0.1 * 0.1) + 0.1 * 0.1


# ---- unbiasedness and calibration against the oracle ------------------------------------------------------------------------
def oracle_chunk_frames(oracle, t, seeds):
    scene, cam = t.scene_desc(), t.camera_desc()
    frames = []
    for seed in seeds:
        p = capi.RenderParams.from_buffer_copy(bytes(t.params()))
        p.seed, p.samples_per_px, p.chunk_spp = seed, 16, 16
        frames.append(oracle.render_b(scene, cam, p)[0])
    return np.stack(frames)


def test_the_estimate_is_calibrated_on_the_oracle(oracle):
    """The oracle exposes no chunk sums, so independent ones are built: 16-sample frames of random_bouncing at 48x27 under
    different seeds, x 16 (exact) — the 16 chunk sums of one 256-sample estimate.  z = (mean - ref) / sqrt(var + var_ref) per
    channel against 4096 samples built the same way has a robust sigma near 1.03 (Student's t, 15 degrees of freedom) if var is
    the variance of the mean.  Measured when the band was recorded, 8 seed sets: 1.0406 1.0264 0.9757 1.0593 1.0069 1.0241 1.0492
    1.0214 — mean 1.0255, spread 0.0261 (noise_ref.Z_SIGMA_*)."""
    t = tracer.randomBouncing(48, seed=7)
    t.samples_per_px, t.max_bounces = 16, 12
    t.set_gpu(render_seed=11)
    ref = oracle_chunk_frames(oracle, t, [1_000_000 + k for k in range(256)])
    vals = []
    for s in range(8):
        frames = oracle_chunk_frames(oracle, t, [1000 * (s + 1) + k for k in range(16)])
        vals.append(noise_ref.z_sigma(frames, ref, 16))
    print("z sigma per seed set:", " ".join(f"{v:.4f}" for v in vals), f"mean {np.mean(vals):.4f} spread {np.std(vals, ddof=1):.4f}")
    lo, hi = noise_ref.Z_SIGMA_BAND
    assert all(lo <= v <= hi for v in vals), (vals, lo, hi)
    assert abs(np.mean(vals) - 1.03) < 0.05  # and the mean sits where Student's t puts it
