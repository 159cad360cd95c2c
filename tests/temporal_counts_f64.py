"""DESIGN.md §4.23 (the counts step, plain and moments) in numpy float64, written from the section's text and not from
tests/temporal_counts_mirror.cpp or the kernel header.  §4.23 changes things INSIDE §4.15's gather and blend, so it is no wrapper:
`temporal_f64.TemporalF64.step` and `temporal_moments_f64.TemporalMomentsF64.step` take `spp` as one number or as an (h, w) integer
array, and the rules below are switched on only for an array; the scalar step is what it was (tests/test_temporal_counts_f64_cpu.py:
an array of one value gives the scalar step's values, bounds and masks exactly).  This module names the statement, lists the wrong
readings, and holds outputs to it (`within_bound`).

What the array switches on, with the bound of each (u = 2^-24, first order, DOUBLED where reported or used as a margin; δh, δhv,
δhN, δhq, δhW are §4.15's gather bounds with the record's own carried E):

  Count.   n = f32(count) is exact for counts up to 2^24 (asserted).  n > 0 compares integers: no margin.
  Rule 1.  A tap is accepted only if, besides §4.15's tests, N_prev(q) > 0 — the static step's one tap too.  A refused tap adds
           nothing to B, H or any other sum.  A record's length is 0 exactly (rule 2 stored a count of 0 by selection) or positive;
           the decision is treated like every other: a pixel is `near` where a relevant tap (b > 0 or δb > 0, same index, inside)
           has 0 < N_prev(q) <= 2·EN(q).  The CPU test asserts that this never fires on the listed inputs.
  Rule 2.  No history: c_out = c, v_out = clamp(s), N_out = n, bound 0.  Where n = 0 the input may be a NaN and passes through; such
           a value is compared by equality with NaN equal to NaN (`passthrough`), not by |d| <= 0.
  Rule 3.  History, n > 0: §4.15 step 4 with n for spp; the bounds are §4.15's with n per pixel.
  Rule 4.  History, n = 0: al = 0 BY SELECTION — a0 < am is not decided and has no margin; the input is never read (the reference
           selects with `np.where` on the value, it does not multiply a NaN by 0).  c_out = h (δh), v_out = hv (δhv),
           N_out = hN > nm ? nm : hN (δhN, margin 2·δhN on the nm decision).
  Rule 5.  Background as §4.15: the input, N_out = n.
  Moments. The same for m2 and W2: with history and n = 0, m2_out = hq (δhq) and W2_out = hW (δhW); §4.16 steps 3 and 5 run on
           those.  Step 4's neighbourhood counts a position q only if count_q > 0, and the centre only if n_p > 0; S0 and the
           bound terms that grow with S0 run over the counted taps.

NaN hygiene.  Histories and inputs hold NaN at unsampled pixels by design.  Every sum selects its records before it weighs them.  A
NaN in an output, bound or mask of the reference at a pixel whose record holds samples (N_out > 0) is a bug of the reference;
`no_nan_where_sampled` asserts there is none."""
import numpy as np

import temporal_f64
import temporal_moments_f64
from temporal_f64 import TemporalF64  # noqa: F401
from temporal_moments_f64 import NAMES, TemporalMomentsF64  # noqa: F401

PLAIN_MISREADINGS = temporal_f64.COUNTS_MISREADINGS
MOMENTS_MISREADINGS = temporal_moments_f64.COUNTS_MISREADINGS
COUNTS_MISREADINGS = PLAIN_MISREADINGS + MOMENTS_MISREADINGS
# zero_length_record_accepted: rule 1 is not applied.  zero_length_tap_in_B: the tap is refused but its weight stays in B.
# static_tap_exempt_from_length_test: the static step's one tap skips rule 1.  alpha_min_applied_at_zero_count: al = max(0, am) where
# n = 0, and the blend runs on the input.  zero_count_takes_input: n = 0 with history gives c_out = c, v_out = s.
# zero_count_resets_length: N_out = n = 0 there.  length_uncapped_at_zero_count: N_out = hN there, whatever nm.
# variance_from_input_at_zero_count: v_out = s there.  count_shared_over_the_frame: one n for all pixels, the frame's mean count.
# background_keeps_history: a background pixel of the default mode takes its own record.  neighbourhood_counts_unsampled: the 7x7 runs
# over unsampled positions too.  centre_counted_without_samples: the centre is counted whatever n_p.  m2_from_input_at_zero_count:
# m2_out = c·c where n = 0 with history.  w2_reset_at_zero_count: W2_out = 1 there.  w2_blended_at_zero_count: W2_out = k²·hW + al² with
# al = alpha_min there.

# The draws.  On integer lengths — a static step, or a moved one that accepts one tap — the decisions of the blend have exact
# solutions: N = n gives al = 1/2 and, over a record that never blended, W2 = 1/2, the tests' w2_max; N = 1.5·n gives a0 = 0.4 and
# N + n = 20 gives Ns = 20, alpha_min and n_max of their binding set; and a record that has reached n_max sits ON that border at
# every later step without samples, and taints what reads it.  A reference cannot hold such pixels, so the inputs avoid them: every
# frame draws its counts from its own values, the values odd from the second frame on (1.5·n is no length) and with no N = n and no
# N + n = 20 among the sums of earlier frames before the last step.  LONG, beyond that n_max, goes to ONE hit pixel of the first
# frame, which the second frame leaves without samples: rule 2 stores 32 uncapped and rule 4 caps what it keeps.
DRAWS = ((1, 2), (5,), (7,), (3,), (9,))
LONG = 32
ZERO = 0.4  # the share of a frame's pixels without samples, as two of the five values of {0, 0, 1, 4, 8}


def sparse(frames, seed):
    """The frames with per-pixel counts ("counts") that are 0 at two pixels in five and one of the frame's own DRAWS at the others, one hit pixel of the first frame
    set to 32 and of the second to 0, and NaN colour and variance wherever the count is 0 — what a sparse render leaves where it
    traced nothing."""
    rng = np.random.default_rng(seed)
    out = []
    hits = np.argwhere(frames[0]["index"] >= 0)
    long = hits[rng.choice(len(hits), 1)] if len(frames) > 1 and len(hits) else hits[:0]
    for k, f in enumerate(frames):
        counts = rng.choice(np.array(DRAWS[k % len(DRAWS)]), size=f["index"].shape).astype(np.int32)
        counts[rng.random(counts.shape) < ZERO] = 0
        if k < 2:
            counts[long[:, 0], long[:, 1]] = LONG if k == 0 else 0
        rgb, var = f["rgb"].copy(), f["var"].copy()
        rgb[counts == 0] = np.nan
        var[counts == 0] = np.nan
        out.append(dict(f, rgb=rgb, var=var, counts=counts))
    return out


def no_nan_where_sampled(ref, what):
    """`ref` is what a step returned with bound=True: no NaN in a value or a bound at a pixel whose record holds samples."""
    moments = isinstance(ref[-1], tuple)
    vals, bnds = (ref[:4], ref[4]) if moments else (ref[:3], ref[3])
    live = vals[2] > 0
    for name, x in zip(NAMES + tuple("bound of " + n for n in NAMES), tuple(vals) + tuple(bnds)):
        bad = np.isnan(x) & (live if x.ndim == 2 else live[..., None])
        assert not bad.any(), f"{what}: NaN in the reference's {name} at {np.argwhere(bad)[:3].tolist()}, a pixel whose record holds samples"
    assert not np.isnan(vals[2]).any(), what


def within_bound(got, ref, hit, what, passthrough, region=None, cap=0.02):
    """Holds one counts step's f32 outputs `got` — plain: (colour, variance[, length]); moments: (colour, variance[, length, W2]) —
    to `ref`, what `step(..., bound=True)` returned for the same inputs, and to `passthrough`, the reference's `last_passthrough`
    of that step.  At most `cap` of the `hit` pixels in each exclusion mask.  Within `region` (every pixel if None), outside the
    mask: a value the reference holds by selection from the inputs (`passthrough`: colour, length, W2, and a plain step's
    variance) equals it with NaN equal to NaN; every other value lies within its bound.  Returns (the largest |difference| / bound
    per output, the excluded shares, the number of values compared by equality)."""
    moments = isinstance(ref[-1], tuple)
    if moments:
        vals, bnds, (ex, vex) = ref[:4], ref[4], ref[5]
    else:
        vals, bnds, ex = ref[:-2], ref[-2], ref[-1]
        vex = ex
    assert len(got) <= len(vals) and len(got) >= 2, what
    region = np.ones(ex.shape, bool) if region is None else region
    nhit = max(int(hit.sum()), 1)
    shares = (float(ex[hit].sum()) / nhit, float(vex[hit].sum()) / nhit)
    assert not ex[~hit].any() and not vex[~hit].any(), what
    assert max(shares) <= cap, f"{what}: {int(ex.sum())} (variance: {int(vex.sum())}) of {int(hit.sum())} hit pixels excluded (cap {cap})"
    assert passthrough.shape == ex.shape and not (passthrough & ex).any(), what
    ratios, equal = [], 0
    for name, g, x, b in zip(NAMES, got, vals, bnds):
        out = vex if name == "variance" else ex
        by_selection = passthrough & (not (moments and name == "variance"))
        wide = (lambda m: m) if g.ndim == 2 else (lambda m: np.broadcast_to(m[..., None], g.shape))
        keep, same = wide(region & ~out & ~by_selection), wide(region & ~out & by_selection)
        g64 = np.asarray(g, np.float64)
        with np.errstate(invalid="ignore"):
            d = np.abs(g64 - x)
            bad = np.argwhere((keep & ~(d <= b)) | (same & ~((g64 == x) | (np.isnan(g64) & np.isnan(x)))))
        assert len(bad) == 0, f"{what} {name}: {len(bad)} values outside the bound; first at {bad[:3].tolist()}: " \
                              f"{[(float(g[tuple(i)]), float(x[tuple(i)]), float(b[tuple(i)]), bool(wide(by_selection)[tuple(i)])) for i in bad[:3]]}"
        equal += int(same.sum())
        with np.errstate(all="ignore"):
            ratios.append(float(np.where(d == 0, 0.0, d / b)[keep].max()) if keep.any() else 0.0)
    return ratios, shares, equal
