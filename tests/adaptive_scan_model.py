"""A model of the ordered compaction of adaptive passes (DESIGN.md §4.14 "Device side"; the comments of rayz_amd/csrc/adaptive.hpp),
in numpy, with the ways the three kernels could be misread as switches.

What the comments say.  The list is cut into blocks of 256 entries, four waves of 64 lanes.  The fold counts each block's
survivors: entries below n_active whose pixel is still active.  One workgroup of 1,024 threads (16 waves of 64 lanes) turns the
counts into exclusive prefix sums, 1,024 counts per round: a count's offset is the running carry of the rounds before, plus the
totals of the earlier waves of its round, plus the counts of the earlier lanes of its wave; the carry then grows by the round's
total, and after the last round it is the new n_active.  The scatter sends a surviving entry to its block's offset plus the
survivor counts of the block's earlier waves plus its rank among its own wave's survivors, so the old order is kept.

compact(entries, survives, misreading) returns the next list and the total as a device with that misreading would leave them: the
next list starts as SENTINEL everywhere (capacity: the old list's length plus a block), stores land where the misreading sends
them (the later entry wins a slot two entries share; a store beyond the capacity is dropped and counted), and the list is the
first `total` slots.  No misreading: the ordered compaction.

The scan misreadings — no_wave_sums, no_carry, carry_exclusive, carry_not_accumulated — change nothing until there are more than
64 blocks (the first two waves) or more than 1,024 (the carry), which tests/test_adaptive_masks_cpu.py keeps as a test."""
import numpy as np

BLOCK, WAVE, SCAN_WAVES = 256, 64, 16
ROUND = SCAN_WAVES * WAVE
SENTINEL = np.uint32(0xFFFFFFFF)

MISREADINGS = (
    "no_wave_sums",                   # scan: a count's offset leaves the earlier waves' totals out
    "wave_sums_inclusive",            # scan: .. or takes its own wave's total too
    "no_carry",                       # scan: .. or leaves the carry out
                                      # (under these three, and under carry_not_accumulated, the total is still right: the
                                      # host's `left > n_active` guard sees nothing)
    "carry_exclusive",                # scan: the carry is the last thread's EXCLUSIVE value: the round's last count is lost
    "carry_not_accumulated",          # scan: the carry is the round's own total: wrong only from the third round
    "total_from_last_round",          # scan: n_active is the last round's total, offsets are right
    "rank_inclusive",                 # scatter: a lane counts itself
    "scatter_wave_counts_inclusive",  # scatter: a wave adds its own survivor count too
    "tail_lanes_counted",             # fold and scatter: lanes at or beyond n_active count as survivors
)
SCAN_MISREADINGS = ("no_wave_sums", "no_carry", "carry_exclusive", "carry_not_accumulated")


def _lanes(survives, n_active, tail):
    """survivor flags per lane, (blocks, 4 waves, 64 lanes): the list padded to whole blocks."""
    blocks = -(-n_active // BLOCK)
    lanes = np.full(blocks * BLOCK, bool(tail))
    lanes[:n_active] = survives
    return lanes.reshape(blocks, BLOCK // WAVE, WAVE)


def scan(counts, mis=None):
    """Exclusive offsets of the block counts and the total, by rounds of 1,024 counts x 16 waves x 64 lanes."""
    n = len(counts)
    rounds = -(-n // ROUND)
    v = np.zeros(rounds * ROUND, dtype=np.int64)
    v[:n] = counts
    v = v.reshape(rounds, SCAN_WAVES, WAVE)
    in_wave = np.cumsum(v, axis=2)                        # inclusive, over the lanes of a wave
    wave_total = in_wave[:, :, -1]
    earlier = np.cumsum(wave_total, axis=1) - wave_total  # the waves before, within the round
    if mis == "no_wave_sums":
        earlier = np.zeros_like(earlier)
    elif mis == "wave_sums_inclusive":
        earlier = earlier + wave_total
    offsets = np.zeros_like(v)
    carry = total = 0                                     # (the carry the offsets use, and the one that becomes n_active)
    for r in range(rounds):                               # (a loop over rounds, at most a handful)
        before = earlier[r] + (0 if mis == "no_carry" else carry)
        offsets[r] = before[:, None] + in_wave[r] - v[r]
        end = v[r].sum()                                  # the round's total: what its last thread holds, without the carry
        if mis == "carry_exclusive":
            end -= v[r, -1, -1]
        carry = end if mis == "carry_not_accumulated" else carry + end
        total = end if mis == "total_from_last_round" else total + end
    return offsets.reshape(-1)[:n], int(total)


def compact(entries, survives, mis=None):
    """-> next list (uint32, `total` long, SENTINEL where nothing was stored), total, stores dropped beyond the capacity."""
    assert mis is None or mis in MISREADINGS
    entries = np.asarray(entries, dtype=np.uint32)
    n_active = len(entries)
    lanes = _lanes(np.asarray(survives, dtype=bool), n_active, mis == "tail_lanes_counted")
    offsets, total = scan(lanes.sum(axis=(1, 2)), mis)
    wave_count = lanes.sum(axis=2)
    waves_before = np.cumsum(wave_count, axis=1) - (0 if mis == "scatter_wave_counts_inclusive" else wave_count)
    rank = np.cumsum(lanes, axis=2) - (0 if mis == "rank_inclusive" else lanes)
    at = (offsets[:, None, None] + waves_before[:, :, None] + rank).reshape(-1)
    padded = np.zeros(lanes.size, dtype=np.uint32)        # (a tail lane that stores, stores pixel 0)
    padded[:n_active] = entries
    who = lanes.reshape(-1)
    capacity = n_active + BLOCK
    nxt = np.full(capacity, SENTINEL)
    at, val = at[who], padded[who]
    inside = at < capacity
    nxt[at[inside]] = val[inside]                         # (numpy keeps the last of the stores to one slot)
    return nxt[:min(max(total, 0), capacity)], total, int(np.count_nonzero(~inside))
