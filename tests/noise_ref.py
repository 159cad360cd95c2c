"""DESIGN.md §4.12 in numpy: the noise estimate of a progressive render, f64 with + - x / only.

Written from the section's text, not from the kernels.  numpy's float64 operators are the IEEE operations, correctly rounded, and
numpy never contracts a multiply and an add, so every value below is the value the contract defines, bit for bit.

    fold(chunk_sums, chunk_sizes, precision)  ->  M (the accumulator, widened), Q
    evaluate(M, Q, K, N, rel_error, mean_floor)  ->  var, rel2, summary
"""
from __future__ import annotations

import math

import numpy as np

DEFAULT_REL_ERROR, DEFAULT_MEAN_FLOOR = 0.05, 0.02

# The calibration statistic z_sigma() measured on the CPU oracle (tests/test_noise_cpu.py: random_bouncing at 48x27, 16 chunks
# of 16 samples against 4096 samples, 8 seed sets): mean and seed-to-seed standard deviation.  Student's t with 15 degrees of
# freedom gives 1.03.  The band both calibration tests assert: mean +- max(0.1, 4 x spread).
Z_SIGMA_MEAN, Z_SIGMA_SPREAD = 1.0255, 0.0261
Z_SIGMA_BAND = (Z_SIGMA_MEAN - max(0.1, 4 * Z_SIGMA_SPREAD), Z_SIGMA_MEAN + max(0.1, 4 * Z_SIGMA_SPREAD))


def fold(chunk_sums, chunk_sizes, f64: bool = False):
    """chunk_sums (K, n, 3) float64, narrowed to the precision R as they cross the interface; chunk_sizes (K,) samples per chunk.
    acc starts at +0 and adds the chunk sums in chunk order in R; Q starts at +0 and adds (t·t)/n_k, t = the chunk sum widened."""
    R = np.float64 if f64 else np.float32
    s = np.asarray(chunk_sums, dtype=np.float64).astype(R)
    K, n, _ = s.shape
    acc = np.zeros((n, 3), dtype=R)
    Q = np.zeros((n, 3), dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(K):
            acc = acc + s[k]
            t = s[k].astype(np.float64)
            Q = Q + (t * t) / np.float64(chunk_sizes[k])
    return acc.astype(np.float64), Q


def evaluate(M, Q, K: int, N: int, rel_error: float = DEFAULT_REL_ERROR, mean_floor: float = DEFAULT_MEAN_FLOOR):
    """var, rel2 (float64, one per pixel) and the summary dict after K chunks and N samples."""
    M, Q = np.asarray(M, dtype=np.float64), np.asarray(Q, dtype=np.float64)
    n = M.shape[0]
    tau2, floor2 = np.float64(rel_error) * np.float64(rel_error), np.float64(mean_floor) * np.float64(mean_floor)
    Nf, Kf = np.float64(N), np.float64(K)
    with np.errstate(all="ignore"):
        if K < 2:
            var = np.full(n, np.inf)
            rel2 = np.full(n, np.inf)
        else:
            D = Q - (M * M) / Nf
            D = np.where(D < 0, 0.0, D)  # (a NaN compares false and stays)
            var = ((D[:, 0] + D[:, 1]) + D[:, 2]) / ((Kf - 1.0) * Nf)
            m2 = ((M[:, 0] * M[:, 0] + M[:, 1] * M[:, 1]) + M[:, 2] * M[:, 2]) / (Nf * Nf)
            den = np.where(m2 > floor2, m2, floor2)
            rel2 = var / den
        unconverged = int(np.count_nonzero(~(rel2 <= tau2)))
    # the maximum by bit pattern with the sign bit cleared: a NaN's pattern sorts above +inf's
    bits = rel2.view(np.uint64) & np.uint64(0x7FFFFFFFFFFFFFFF)
    max_rel2 = float(np.array([bits.max()], dtype=np.uint64).view(np.float64)[0]) if n else 0.0
    finite = var[np.isfinite(var)]
    mean_var = math.fsum(finite.tolist()) / n if n else 0.0  # (the order of this sum is not part of the contract: compare to 1e-12)
    return var, rel2, {"pixels": n, "unconverged": unconverged, "max_rel2": max_rel2, "mean_var": mean_var,
                       "samples_done": int(N), "chunks_done": int(K)}


def estimate(chunk_sums, chunk_sizes, f64: bool = False, rel_error: float = DEFAULT_REL_ERROR, mean_floor: float = DEFAULT_MEAN_FLOOR):
    """fold + evaluate: (Q, var, rel2, summary) of the whole list of chunks."""
    M, Q = fold(chunk_sums, chunk_sizes, f64)
    K, N = len(chunk_sizes), int(np.sum(np.asarray(chunk_sizes, dtype=np.uint64)))
    var, rel2, summary = evaluate(M, Q, K, N, rel_error, mean_floor)
    return Q, var, rel2, summary


def z_sigma(chunk_frames, ref_chunk_frames, chunk_spp: int):
    """The calibration statistic of §4.12 / §6: chunk_frames (K, h, w, 3) are K independent chunk_spp-sample frames (means) of one
    image, ref_chunk_frames (Kr, h, w, 3) those of a much longer reference estimate.  Per channel z = (mean - ref) /
    sqrt(var_ch + var_ref_ch) with both variances from the chunk-sum estimate; returns the robust sigma (IQR / 1.349) of z over all
    pixels and channels where the denominator is positive.  A calibrated estimate gives about 1.03 at K = 16 (Student's t, 15
    degrees of freedom)."""
    def mean_and_var(frames):
        f = np.asarray(frames, dtype=np.float64)
        K = f.shape[0]
        S = f.reshape(K, -1, 3) * chunk_spp  # chunk sums
        N = K * chunk_spp
        M = S.sum(axis=0)
        Q = (S * S / chunk_spp).sum(axis=0)
        D = np.maximum(Q - M * M / N, 0.0)
        return M / N, D / ((K - 1) * N)  # per channel: the variance of the mean

    m, v = mean_and_var(chunk_frames)
    mr, vr = mean_and_var(ref_chunk_frames)
    den = v + vr
    ok = den > 0
    z = (m - mr)[ok] / np.sqrt(den[ok])
    q75, q25 = np.percentile(z, [75, 25])
    return float((q75 - q25) / 1.349)


def z_sigma_from_moments(M, Q, K, N, Mr, Qr, Kr, Nr):
    """z_sigma() from the state itself: accumulators M (n, 3) and moments Q (n, 3) after K chunks / N samples of an estimate and
    of a longer, independent reference estimate."""
    def mean_and_var(M, Q, K, N):
        M, Q = np.asarray(M, dtype=np.float64), np.asarray(Q, dtype=np.float64)
        return M / N, np.maximum(Q - M * M / N, 0.0) / ((K - 1) * N)

    m, v = mean_and_var(M, Q, K, N)
    mr, vr = mean_and_var(Mr, Qr, Kr, Nr)
    den = v + vr
    ok = den > 0
    z = (m - mr)[ok] / np.sqrt(den[ok])
    q75, q25 = np.percentile(z, [75, 25])
    return float((q75 - q25) / 1.349)
