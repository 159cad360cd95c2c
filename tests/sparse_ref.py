"""DESIGN.md §4.21 in numpy: what a sparse render makes of the chunk sums of its listed pixels.

Written from the section's text, not from the kernel.  Entry j has one chunk sum per chunk of the frame's schedule; its colour is
those sums added in chunk order from +0 in the render's precision R, times R(1) / R(spp); its per-channel variance is §4.12's
D_ch / ((K - 1) · N) on Q_ch = sum of (t · t) / n_k (t the chunk sum widened to float64), rounded once to float32, +inf for
K < 2.  Entry j lands in slot dest[j] (j without dest); slots nobody names keep what they held.

    resolve(chunk_sums, chunk_sizes, f64=False, dest=None, out=None, var=None)  ->  out, var
"""
from __future__ import annotations

import numpy as np


def resolve(chunk_sums, chunk_sizes, f64: bool = False, dest=None, out=None, var=None):
    """chunk_sums (K, n, 3), narrowed to R as they cross the interface; chunk_sizes (K,).  `out` (slots, 3) of R and `var`
    (slots, 3) float32 are updated in place where given (new (n, 3) arrays otherwise) and returned."""
    R = np.float64 if f64 else np.float32
    s = np.asarray(chunk_sums, dtype=np.float64).astype(R)
    K, n, _ = s.shape
    N = int(np.sum(np.asarray(chunk_sizes, dtype=np.uint64)))
    x = np.zeros((n, 3), dtype=R)
    Q = np.zeros((n, 3), dtype=np.float64)
    with np.errstate(all="ignore"):
        for k in range(K):
            x = x + s[k]
            t = s[k].astype(np.float64)
            Q = Q + (t * t) / np.float64(chunk_sizes[k])
        colour = x * (R(1) / R(N))
        if K < 2:
            v = np.full((n, 3), np.inf, dtype=np.float32)
        else:
            M = x.astype(np.float64)
            D = Q - (M * M) / np.float64(N)
            D = np.where(D < 0, 0.0, D)  # (a NaN compares false and stays)
            v = (D / ((np.float64(K) - 1.0) * np.float64(N))).astype(np.float32)
    slot = np.arange(n) if dest is None else np.asarray(dest, dtype=np.int64)
    out = np.empty((n, 3), dtype=R) if out is None else out
    var = np.empty((n, 3), dtype=np.float32) if var is None else var
    out[slot] = colour
    var[slot] = v
    return out, var
