"""The designed freeze maps and the compaction model, without a GPU (tests/adaptive_masks.py, tests/adaptive_scan_model.py).

1. Every map tests/test_adaptive_sizes_gpu.py uses is reproduced exactly by adaptive_ref in f32 and in f64: each pixel freezes at
   its designed pass and the lists are the ones the map alone gives.  A condition on the inputs; no pixel is left out.
2. The model of the three compaction kernels equals those lists on every case, and every named misreading of the kernels gives a
   different list or total on at least one of them: CAUGHT_BY names, per misreading, cases that must catch it (the whole table is
   printed: pytest -s).
3. The statement of the gap those cases close: the four scan misreadings equal the truth at every size the suite ran before."""
import numpy as np
import pytest

import adaptive_masks as masks
import adaptive_ref
import adaptive_scan_model as model


@pytest.mark.parametrize("n, width, name", masks.CASES, ids=masks.CASE_IDS)
def test_adaptive_ref_freezes_every_pixel_at_its_designed_pass(n, width, name):
    c = masks.case(n, width, name)
    for f64 in (False, True):
        r = adaptive_ref.run(c["sums"], c["sizes"], c["ends"], f64=f64, min_chunks=masks.MIN_CHUNKS, width=width)
        assert np.array_equal(r["frozen_at"], c["F"]), (f64, np.flatnonzero(r["frozen_at"] != c["F"])[:4])
        assert np.array_equal(r["counts"], c["counts"])
        assert len(r["lists"]) == c["K"] + 1
        for p, (g, w) in enumerate(zip(r["lists"], c["lists"])):
            assert np.array_equal(g, w), (f64, p)
    # .. and the case is the one its name claims: the first pass that freezes compacts a list beyond the threshold, to a list that
    # is neither empty nor whole (nobody_freezes: whole, every time)
    before, after = len(c["lists"][1]), len(c["lists"][2])
    assert len(c["lists"][0]) == before == n > masks.claim(n)
    if name == "nobody_freezes":
        assert all(np.array_equal(l, c["lists"][0]) for l in c["lists"])
    else:
        assert 0 < after < before
    if name == "random":
        left = [len(l) for l in c["lists"]]
        assert all(0.15 * n < a - b < 0.25 * n for a, b in zip(left[1:], left[2:])) and 0.15 * n < left[-1] < 0.25 * n
        assert c["F"][c["nan"][0]] == 0 and np.isnan(c["sums"][0, c["nan"][0], 1]) and (c["sums"][:, c["black"][0]] == 0).all()


# Cases that must catch each misreading, by where their survivors sit (positions in the compacted list):
CAUGHT_BY = {
    # survivors in block 64 or beyond BEHIND survivors in blocks 0 - 63: its offset is the total of the scan's first wave
    # (wave0_freezes and wave0_survives put survivors on one side only: the first wave's total, or what follows it, is 0)
    "no_wave_sums": ["16385-nobody_freezes", "16385-random", "16640-random", "262144-stripes"],
    "wave_sums_inclusive": ["16384-only_16383", "16384-random"],
    # a survivor in round two behind survivors in round one
    "no_carry": ["262145-nobody_freezes", "262145-one_per_round", "524545-one_per_round", "524545-random"],
    # block 1,023 holds survivors and something follows it (an entry of round two, or the total itself)
    "carry_exclusive": ["262144-last_block_of_round_one", "262144-only_262143", "262145-random"],
    # a third round behind survivors in round one
    "carry_not_accumulated": ["524545-random", "524545-one_per_round", "524545-nobody_freezes"],
    "total_from_last_round": ["262145-random", "262145-only_0", "524545-one_per_round"],
    "rank_inclusive": ["16384-only_0", "16384-last_entry", "524545-random"],
    "scatter_wave_counts_inclusive": ["16384-only_0", "16384-stripes"],
    # sizes that are no multiple of 256
    "tail_lanes_counted": ["16385-random", "262145-only_0", "524545-stripes"],
}


@pytest.fixture(scope="module")
def table():
    """{misreading: [case ids that give a different list or total]}, after checking the unswitched model on every pass of every
    case.  A misreading is tried on the passes that can freeze and whose list is longer than a block."""
    caught = {m: [] for m in model.MISREADINGS}
    for (n, width, name), cid in zip(masks.CASES, masks.CASE_IDS):
        c = masks.case(n, width, name)
        hit = set()
        for p, end in enumerate(c["ends"]):
            cur, want = c["lists"][p], c["lists"][p + 1]
            survives = c["F"][cur] != end
            got, total, dropped = model.compact(cur, survives)
            assert total == len(want) and dropped == 0 and np.array_equal(got, want), (cid, p)
            if p == 0 or len(cur) <= model.BLOCK:  # (pass 0 freezes nobody in every case: nobody_freezes speaks for it)
                continue
            for m in model.MISREADINGS:
                if m not in hit:
                    got, total, _ = model.compact(cur, survives, m)
                    if total != len(want) or not np.array_equal(got, want):
                        hit.add(m)
        for m in hit:
            caught[m].append(cid)
    return caught


def test_the_model_equals_the_designed_lists_and_every_misreading_is_caught(table):
    print()
    for m in model.MISREADINGS:
        every = len(table[m]) == len(masks.CASES)
        print(f"{m}: {len(table[m])} of {len(masks.CASES)} cases" + ("" if every else ": " + " ".join(table[m])))
    assert set(CAUGHT_BY) == set(model.MISREADINGS)
    for m, named in CAUGHT_BY.items():
        assert named and set(named) <= set(table[m]), (m, sorted(set(named) - set(table[m])))
    # the carry's misreadings need the sizes they were chosen for: nothing at or below one round sees them
    for m in ("no_carry", "carry_not_accumulated"):
        assert all(int(cid.split("-")[0]) > masks.ROUND_ENTRIES for cid in table[m]), m
    assert all(int(cid.split("-")[0]) > 2 * masks.ROUND_ENTRIES for cid in table["carry_not_accumulated"])
    assert all(int(cid.split("-")[0]) > masks.WAVE_ENTRIES for cid in table["no_wave_sums"])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 300, 480, 1000, 5184])
def test_the_scan_misreadings_were_invisible_at_every_size_the_suite_ran(n):
    """The sizes of tests/test_adaptive_gpu.py's known-answer runs and of the largest adaptive handle in the suite (96x54): at most
    21 blocks, so one wave of one round.  Random masks of every density, all and none."""
    rng = np.random.default_rng(n)
    entries = rng.permutation(n).astype(np.uint32)
    for density in (0.0, 0.03, 0.5, 0.97, 1.0):
        survives = rng.random(n) < density
        want = entries[survives]
        for m in (None,) + model.SCAN_MISREADINGS:
            got, total, dropped = model.compact(entries, survives, m)
            assert total == len(want) and dropped == 0 and np.array_equal(got, want), (m, density)
