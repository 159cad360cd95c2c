"""DESIGN.md §4.14 in numpy: adaptive passes over caller chunk sums.

Written from the section's text, not from the kernels; §4.12's arithmetic comes from its own restatement (noise_ref).  numpy's
float32 / float64 operators are the IEEE operations, correctly rounded, never contracted, so every value is the contract's.

    deal_order(n_pixels, width)  ->  the order pixels are dealt (the first active list)
    run(chunk_sums, chunk_sizes, pass_ends, ...)  ->  frozen_at, acc, Q, frame, counts, lists
"""
from __future__ import annotations

import numpy as np

import noise_ref

DEFAULT_MIN_CHUNKS = 4


def deal_order(n_pixels: int, width: int = 0) -> np.ndarray:
    """Row-major local pixel indices in dealing order: 8x8 tiles over the whole tile rows when width % 8 == 0, tile by tile along
    a tile row and row-major inside a tile, then the remaining pixels row by row.  width 0: 0, 1, 2, .."""
    idx = np.arange(n_pixels, dtype=np.uint32)
    if not width or width % 8:
        return idx
    rows = n_pixels // width
    tiled = rows // 8 * 8 * width
    t = idx[:tiled].reshape(rows // 8, 8, width // 8, 8).transpose(0, 2, 1, 3).reshape(-1)
    return np.concatenate([t, idx[tiled:]])


def run(chunk_sums, chunk_sizes, pass_ends, f64: bool = False, rel_error: float = noise_ref.DEFAULT_REL_ERROR,
        mean_floor: float = noise_ref.DEFAULT_MEAN_FLOOR, min_chunks: int = DEFAULT_MIN_CHUNKS, width: int = 0):
    """chunk_sums (K, n, 3) float64, narrowed to the precision R as they cross the interface; pass p covers the chunks
    [pass_ends[p-1], pass_ends[p]).  Returns a dict: frozen_at (n,) uint32, acc and Q (n, 3) float64 (acc widened), frame (n, 3)
    float64 (the R values widened), counts (n,) = N_i, lists = the active list every pass traced, then what is left."""
    assert min_chunks >= 2
    R = np.float64 if f64 else np.float32
    s = np.asarray(chunk_sums, dtype=np.float64).astype(R)
    K, n, _ = s.shape
    sizes = np.asarray(chunk_sizes, dtype=np.uint64)
    starts = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    acc, Q = np.zeros((n, 3), dtype=R), np.zeros((n, 3), dtype=np.float64)
    frozen_at = np.zeros(n, dtype=np.uint32)
    active = deal_order(n, width)
    lists, c0 = [], 0
    with np.errstate(all="ignore"):
        for c1 in pass_ends:
            if not len(active):  # the run has ended: later passes trace nothing and move no cursor
                lists.append(active.copy())
                continue
            lists.append(active.copy())
            a = active
            for k in range(c0, c1):  # fold, chunk order, active pixels only
                acc[a] = acc[a] + s[k, a]
                t = s[k, a].astype(np.float64)
                Q[a] = Q[a] + (t * t) / np.float64(sizes[k])
            _, rel2, _ = noise_ref.evaluate(acc[a].astype(np.float64), Q[a], int(c1), int(starts[c1]), rel_error, mean_floor)
            tau2 = np.float64(rel_error) * np.float64(rel_error)
            freeze = (rel2 <= tau2) if c1 >= min_chunks else np.zeros(len(a), dtype=bool)
            frozen_at[a[freeze]] = c1
            active = a[~freeze]  # ordered compaction
            c0 = int(c1)
        lists.append(active.copy())
        counts = starts[np.where(frozen_at != 0, frozen_at, c0)]
        inv = R(1) / counts.astype(R)
        frame = acc * inv[:, None]
    return {"frozen_at": frozen_at, "acc": acc.astype(np.float64), "Q": Q, "frame": frame.astype(np.float64),
            "counts": counts.astype(np.uint32), "lists": lists, "chunks_done": c0}
