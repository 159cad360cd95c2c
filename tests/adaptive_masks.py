"""Designed freeze maps for adaptive passes: chunk sums in which every pixel freezes at a pass chosen in advance,
or never, so that every pass's survivor mask — and with it every active list — is known without running any estimate.

The schedule is K <= 6 chunks of 16 samples, a pass per chunk (pass_ends = 1 .. K), min_chunks 2 and the default rel_error 0.05
(tau2 = 0.0025) and mean_floor 0.02.  A map F gives each pixel 0 (never freezes) or the pass end 2 .. K it freezes at:

  never      chunk sums 0, 32, 0, 32, .. in all channels.  rel2 = 1 at K = 2, 2 at 3, 1/3 at 4, 3/8 at 5, 0.2 at 6: all far above tau2.
  never, NaN a NaN in the green sum of chunk 0, 16 elsewhere: every rel2 is a NaN and NaN <= tau2 is false (§4.14).
  F = p      chunk 0 is 16 (1 + d), every other chunk 16, all channels alike.  §4.12 at K chunks (N = 16 K): per channel
             D = Q − M²/N = 16 d² (1 − 1/K), so var = 3 D / ((K − 1) N) = 3 d² / K², m2 = 3 (1 + d/K)² and rel2 = (d / (K + d))².
             The pixel freezes at the first K >= 2 with d / (K + d) <= 0.05, that is with d <= K / 19: at p >= 3 iff
             (p − 1)/19 < d <= p/19.  DELTA[p] is the multiple of 1/128 nearest the middle of that interval (16 (1 + d) is then
             exact in f32, and so is every partial sum 16 (k + d)); DELTA[2] = 0 is the calm pixel.  The margin to either
             boundary is about a quarter of a step of 1/19 in d — relative 0.1 or more, against f32 and f64 rounding.
  black      every sum +0: D = 0, m2 = 0 < floor2, rel2 = 0 / floor2 = 0: freezes at 2 on 0.

expected_lists() states the lists from F alone: lists[0] is the dealing order and lists[p + 1] is lists[p] without the entries whose
F equals ends[p], order kept.  Nothing here calls adaptive_ref; tests/test_adaptive_masks_cpu.py holds adaptive_ref to these maps,
every pixel of every case, and tests/test_adaptive_sizes_gpu.py the device.

CASES is the table both use: the sizes at which adaptive_scan_kernel's three levels turn over (64 blocks of 256 entries fill the
first wave, 1,024 blocks fill a round) times the masks that put survivors on either side of those edges.  Positions are positions
in the list of pass 1, the first pass that freezes (= the dealing order: pass 0 has one chunk and no estimate); the survivors of
that pass follow the random map."""
import functools

import numpy as np

from adaptive_ref import deal_order

CHUNK = 16
MIN_CHUNKS = 2
BLOCK, WAVE_BLOCKS, ROUND_BLOCKS = 256, 64, 1024
WAVE_ENTRIES, ROUND_ENTRIES = BLOCK * WAVE_BLOCKS, BLOCK * ROUND_BLOCKS  # 16,384 and 262,144
DELTA = {2: 0.0, 3: 17 / 128, 4: 24 / 128, 5: 30 / 128, 6: 37 / 128}
for _p, _d in DELTA.items():
    assert _p == 2 or (_p - 1) / 19 < _d <= _p / 19
    assert float(np.float32(CHUNK * (1 + _d))) == CHUNK * (1 + _d)


def schedule(K):
    return [CHUNK] * K, list(range(1, K + 1))


def chunk_sums(F, K, nan=(), black=()):
    """(K, n, 3) float64 chunk sums realising the map F (n,) over pixels; `nan` and `black` list pixels of the special classes
    (F must be 0 and 2 there)."""
    F = np.asarray(F)
    assert K <= 6 and ((F == 0) | ((F >= 2) & (F <= K))).all()
    first = np.zeros(len(F))
    for p, d in DELTA.items():
        first[F == p] = CHUNK * (1 + d)
    sums = np.empty((K, len(F), 3))
    sums[:] = np.where(F == 0, 0.0, CHUNK)[None, :, None]
    sums[1::2, F == 0] = 2 * CHUNK
    sums[0] = first[:, None]
    for i in nan:
        assert F[i] == 0
        sums[:, i] = CHUNK
        sums[0, i, 1] = np.nan
    for i in black:
        assert F[i] == 2
        sums[:, i] = 0.0
    return sums


def expected_lists(F, K, width=0):
    """The K + 1 lists (what every pass traces, then what is left) from the map alone."""
    F = np.asarray(F)
    lists = [deal_order(len(F), width)]
    for end in range(1, K + 1):
        cur = lists[-1]
        lists.append(cur[F[cur] != end])
    return lists


def expected_counts(F, K):
    return (CHUNK * np.where(np.asarray(F) != 0, F, K)).astype(np.uint32)


# ---- the cases -------------------------------------------------------------------------------------------------------------------
SIZES = [16384, 16385, 16640, 262144, 262145, 524545]
TILED = {16640: 128, 262144: 512, 704 * 396: 704}  # whole 8x8 tile rows plus (16,640: two) rows dealt as they come; 704x396: 1,089 blocks
F64_SIZES = [16640, 262145, 524545]  # one per regime of the scan


def _random_classes(n, K, rng):
    classes = np.array([0] + list(range(2, K + 1)))
    return classes[rng.integers(0, len(classes), n)]


def _survivor_positions(kind, n):
    """Positions (in the list of pass 1) that survive pass 1 in the structured maps; everything else freezes at 2."""
    j = np.arange(n)
    blk = j // BLOCK
    if kind.startswith("only_"):
        return np.array([int(kind[5:])])
    if kind == "one_per_round":  # entry 131 of block 37 of every round, or the round's last entry where the round is shorter
        return np.minimum(np.arange(0, n, ROUND_ENTRIES) + 37 * BLOCK + 131, n - 1)
    return j[{"stripes": blk % 2 == 1,
              "wave0_freezes": blk >= WAVE_BLOCKS,
              "wave0_survives": blk < WAVE_BLOCKS,
              "last_block_of_round_one": blk == ROUND_BLOCKS - 1,
              "first_block_of_round_two": blk == ROUND_BLOCKS,
              "last_entry": j == n - 1,
              "nobody_freezes": j >= 0}[kind]]


def case_names(n):
    """The masks a size allows (one whose survivors would be nobody or everybody is left out: it would not be what it claims)."""
    names = ["random", "stripes"]
    if n > WAVE_ENTRIES:
        names += ["wave0_freezes", "wave0_survives"]
    if n > ROUND_ENTRIES - BLOCK:
        names.append("last_block_of_round_one")
    if n > ROUND_ENTRIES:
        names.append("first_block_of_round_two")
    names.append("last_entry")
    names += [f"only_{j}" for j in (0, WAVE_ENTRIES - 1, WAVE_ENTRIES, ROUND_ENTRIES - 1, ROUND_ENTRIES) if j < n]
    return names + ["one_per_round", "nobody_freezes"]


CASES = [(n, 0, name) for n in SIZES for name in case_names(n)] + [(n, w, "random") for n, w in TILED.items()]
CASE_IDS = [f"{n}-{name}" + (f"-w{w}" if w else "") for n, w, name in CASES]


def claim(n):
    """The largest of the scan's thresholds that n entries exceed (0: one wave of counts is enough)."""
    return max(t for t in (0, WAVE_ENTRIES, ROUND_ENTRIES, 2 * ROUND_ENTRIES) if t < n)


@functools.lru_cache(maxsize=2)
def case(n, width, name):
    """-> dict: F (n,) over pixels, K, sizes, ends, sums (K, n, 3), lists (expected), counts, nan / black pixels."""
    rng = np.random.default_rng([n, width, sum(map(ord, name))])
    order = deal_order(n, width)
    nan, black = (), ()
    if name == "random":
        K = 5  # never, 2, 3, 4, 5: about one fifth each
        F = _random_classes(n, K, rng)
        nan, black = (int(order[3]),), (int(order[2]),)
        F[nan[0]], F[black[0]] = 0, 2
    else:
        K = 4
        F = np.full(n, 2)
        keep = order[_survivor_positions(name, n)]
        F[keep] = 0 if name == "nobody_freezes" else np.array([0, 3, 4])[rng.integers(0, 3, len(keep))]
        if len(keep) == 1:
            F[keep] = 3  # a single survivor: traced by pass 2, gone after it
    sizes, ends = schedule(K)
    out = {"n": n, "width": width, "name": name, "K": K, "F": F, "sizes": sizes, "ends": ends, "nan": nan, "black": black,
           "sums": chunk_sums(F, K, nan, black), "lists": expected_lists(F, K, width), "counts": expected_counts(F, K)}
    out["sums"].setflags(write=False)
    return out
