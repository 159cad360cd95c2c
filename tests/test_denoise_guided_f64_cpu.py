"""The variance-guided denoiser against a float64 statement of its contract, without a GPU: the CPU mirror
(tests/denoise_guided_mirror.cpp, which the GPU tests hold the kernels to bit for bit) stays within the derived per-value bound of
tests/denoise_guided_f64.py in colour and in variance; every listed misreading of §4.13, switched into the reference, leaves that
bound; the reference reproduces the rational hand cases of tests/denoise_guided_cases.py, agrees with §4.11's float64 statement
where the colour term is off, and gives the closed form §4.13 quotes for the variance channel alone."""
import functools
import itertools
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

import denoise_cases
import denoise_f64
import denoise_guided_cases
import denoise_guided_f64 as g64
import denoise_guided_ref

INF = float("inf")
A = denoise_guided_ref.ALBEDO
SIZES = ((63, 65, 6365, 7), (131, 77, 5, 11))  # (width, height, seed of synthetic(), seed of guided_variance())
LEVELS = (1, 2, 5, 8)
# (flags, sigma_color, normal_power_log2, var_floor) at sigma_plane 0.3: both flag states meet every sigma_color, both powers and
# both floors; the floors are four decades apart, above and below most of guided_variance()'s values
COMBOS = [dict(flags=f, sigma_color=sc, normal_power_log2=k, var_floor=vf, sigma_plane=0.3) for f, sc, k, vf in (
    (A, 2.0, 6, 1e-4), (0, 2.0, 6, 1e-4), (A, 0.5, 0, 1e-8), (0, 0.5, 6, 1e-8), (A, INF, 6, 1e-4), (0, INF, 0, 1e-8), (A, 2.0, 0, 1e-8),
    (0, 0.5, 0, 1e-4), (A, 0.5, 6, 1e-4), (0, 2.0, 0, 1e-8))]
EXCLUDED_CAP = 0.001
POOL = max(1, min(8, os.cpu_count() or 1))


@functools.lru_cache(maxsize=None)
def inputs(size):
    w, h, seed, vseed = SIZES[size]
    rgb, index, normal, point, albedo = denoise_cases.synthetic(w, h, seed)
    return rgb, denoise_guided_cases.guided_variance(rgb, vseed), index, normal, point, albedo


@functools.lru_cache(maxsize=None)
def config(size, combo):
    """(mirror results, reference results with bounds) for LEVELS: computed once, shared, never changed."""
    inp, prm = inputs(size), COMBOS[combo]
    mir = denoise_guided_ref.denoise(*inp, levels=8, each_level=True, **prm)
    ref = g64.denoise_guided_f64(*inp, levels=8, want_levels=LEVELS, bound=True, **prm)
    return {L: mir[L - 1] for L in LEVELS}, ref


def _tag(size, combo, L):
    p = COMBOS[combo]
    return (f"{SIZES[size][0]}x{SIZES[size][1]} L={L} flags={p['flags']} sc={p['sigma_color']} k={p['normal_power_log2']} "
            f"vf={p['var_floor']}")


def ratios(got, ref):
    """(largest colour |err| / bound, largest variance |err| / bound) over the pixels the reference does not exclude; a NaN on
    either side of a difference is outside any tolerance (inf)."""
    out, cb, var, vb, excluded = ref
    keep = ~excluded
    with np.errstate(invalid="ignore"):
        rc = np.abs(np.asarray(got[0], np.float64) - out)[keep] / cb[keep]
        rv = np.abs(np.asarray(got[1], np.float64) - var)[keep] / vb[keep]
    return tuple(float("inf") if np.isnan(r).any() else float(r.max()) for r in (rc, rv))


def test_the_mirror_is_within_the_derived_bound_of_the_f64_reference():
    """synthetic() guides and guided_variance() variances (0, tiny, ordinary, 1e12, +inf, NaN, negative) at 63x65 and 131x77; 1, 2, 5
    and 8 levels; ten parameter states: 80 configurations.  Tolerance, per value: the bounds derived in denoise_guided_f64's
    docstring — for the colour §4.11's bound with the pack's and the prefilter's error carried through `den`, for the variance the
    per-term absolute bound of V / (W·W) — both doubled for the second-order terms.  Pixels where the first-order argument fails are
    excluded; at most 0.1 % of a frame may be.  The measured ratios are printed and recorded in DESIGN.md §3; they are not thresholds."""
    jobs = list(itertools.product(range(len(SIZES)), range(len(COMBOS))))
    with ThreadPoolExecutor(POOL) as pool:
        list(pool.map(lambda a: config(*a), jobs))
    worst_c, worst_v, most_excluded = (0.0, ""), (0.0, ""), (0, "")
    for size, combo in jobs:
        mir, ref = config(size, combo)
        for L in LEVELS:
            out, cb, var, vb, excluded = ref[L]
            tag = _tag(size, combo, L)
            assert all(np.isfinite(a).all() for a in (out, cb, var, vb)) and (vb > 0).all() and (var >= 0).all(), tag
            assert excluded.mean() <= EXCLUDED_CAP, (tag, int(excluded.sum()))
            rc, rv = ratios(mir[L], ref[L])
            print(f"mirror vs f64: {tag}: max err/bound colour {rc:.4f}, variance {rv:.4f}, excluded {int(excluded.sum())}")
            worst_c, worst_v = max(worst_c, (rc, tag)), max(worst_v, (rv, tag))
            most_excluded = max(most_excluded, (int(excluded.sum()), tag))
            assert rc <= 1 and rv <= 1, (tag, rc, rv)
    print(f"mirror vs f64, worst err/bound: colour {worst_c[0]:.4f} at {worst_c[1]}; variance {worst_v[0]:.4f} at {worst_v[1]}; "
          + (f"most excluded pixels {most_excluded[0]} at {most_excluded[1]}" if most_excluded[0] else "no pixel excluded anywhere"))


def test_every_misreading_of_the_f64_reference_is_rejected():
    """Each of denoise_guided_f64.MISREADINGS, switched into the reference, must differ from the MIRROR by more than the bound of the
    test above (the reference-as-written's, at the same configuration) in the colour or in the variance at some non-excluded value
    of some configuration — were mirror and kernel to adopt that misreading together, the test above would fail by the same margin.
    Run at 63x65 over all 40 configurations there (the larger frame adds time, not cases).  A misreading that a configuration cannot
    show (the demodulation readings without ALBEDO, the stride and `from_packed` readings at one level, the colour term at
    sigma_color = +inf) is simply not caught THERE; the condition is one catch."""
    size = 0
    inp = inputs(size)

    def one(combo):
        prm = COMBOS[combo]
        mir, ref = config(size, combo)
        rows = {}
        for name in g64.MISREADINGS:
            got = g64.denoise_guided_f64(*inp, levels=8, want_levels=LEVELS, misread=name, **prm)
            for L in LEVELS:
                # the MIRROR against the misread reference, in units of the true reference's bound
                rows[(name, L)] = max(ratios(mir[L], got[L][:1] + ref[L][1:2] + got[L][1:] + ref[L][3:]))
        return rows

    with ThreadPoolExecutor(POOL) as pool:
        rows = list(pool.map(one, range(len(COMBOS))))
    for name in g64.MISREADINGS:
        for combo, r in enumerate(rows):
            print(f"misreading {name}: " + "; ".join(f"{_tag(size, combo, L)}: {r[(name, L)]:.4g}" for L in LEVELS))
        caught = [r[(name, L)] for r in rows for L in LEVELS if r[(name, L)] > 1]
        print(f"misreading {name}: caught in {len(caught)} of {len(rows) * len(LEVELS)} configurations; smallest catch {min(caught, default=0):.4g} x bound, "
              f"largest {max(caught, default=0):.4g} x bound")
        assert caught, f"the misreading {name} stays within the tolerance of the mirror on every input"


# One level of the reference costs, per value: about 15 float64 operations into a tap's weight (each 2^-53 relative, on positive
# factors: the dots of the flat hand guides are exact), a sum of at most 25 like-signed terms (25 roundings at most, whatever order
# np.sum takes), a product and a divide — fewer than 64 roundings, every one on a quantity of one sign, so the relative error of a
# level's value is below 64·2^-53 = 2^-47; the colour weight adds |δwc| / wc <= |δx| with x <= 3 in these cases: below 2^-46 in all.
# The cases run at most two levels, and a level passes its input's relative error on unamplified (a convex mean): 2^-45; 2^-44 leaves
# a factor of two.
REL_F64 = 2.0 ** -44
# `step-vcap` is the case whose rationals CONTAIN two f32 absorptions (tests/denoise_guided_cases.py: 2^32 + 2^-20 = 2^32, and
# 1 + x = 1 for x = 3·2^-32), which float64 does not make: there the reference's wc is 1 / (1 + x) and not 1, |δw| / w <= x < 2^-30, so
# S / W moves by at most 2x and V / (W·W) by at most 4x < 2^-28 relative (den's own shift, 2^-52, is far below).
REL_ABSORBED = 2.0 ** -28


def test_the_reference_reproduces_the_hand_cases():
    """Every case of denoise_guided_cases.cases(): at the pixels `exact()` knows, the reference's demodulated colour and its variance
    equal the rationals to REL_F64 (REL_ABSORBED for `step-vcap`, whose rationals hold f32's absorptions); the three odd_variances()
    packs: a NaN, a +inf and a negative channel give v = VCAP, VCAP and 0 exactly, and every other pixel's v to float64 rounding."""
    for c in denoise_guided_cases.cases():
        rel = REL_ABSORBED if c.name == "step-vcap" else REL_F64
        got = g64.denoise_guided_f64(c.rgb, c.var_rgb, c.index, c.normal, c.point, c.albedo, **c.params)[c.params["levels"]]
        m = g64.pack_f64(c.rgb, c.var_rgb, c.index, c.albedo, flags=c.params["flags"])[0]
        want = denoise_guided_cases.exact(c)
        assert set(c.hand) <= set(want) and want, c.name
        for p, (col, var) in want.items():
            for ch in range(3):
                e = got[0][p][ch] / m[p][ch]  # m is a power of two in every case: exact
                assert abs(e - float(col[ch])) <= rel * abs(float(col[ch])), (c.name, p, ch, e, float(col[ch]))
            assert abs(got[1][p] - float(var)) <= rel * float(var), (c.name, p, got[1][p], float(var))
    for label, c, pixel, v in denoise_guided_cases.odd_variances():
        got = g64.pack_f64(c.rgb, c.var_rgb, c.index, c.albedo, flags=c.params["flags"])[2]
        want = denoise_guided_cases.pack_v(c)
        assert got[pixel] == float(v) == float(want[pixel]), (label, got[pixel], v)
        for p, x in want.items():
            assert abs(got[p] - float(x)) <= 2.0 ** -51 * float(x), (label, p)  # two adds of non-negative terms
        out = g64.denoise_guided_f64(c.rgb, c.var_rgb, c.index, c.normal, c.point, c.albedo, **c.params)[c.params["levels"]]
        assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all(), label


def test_the_two_f64_statements_agree_where_the_colour_term_is_off():
    """sigma_color = +inf: den = +inf, wc = 1, and §4.13's colour is §4.11's — whatever the variance holds (NaN, +inf and negative
    entries included).  Both float64 statements then perform the same real-number operations on the colour: fewer than 100
    roundings of 2^-53 per value and level (see REL_F64), like-signed sums, eight levels each passing its input's error on
    unamplified: below 800·2^-53 < 2^-43 relative; 2^-40 leaves a factor of eight."""
    rgb, var, index, normal, point, albedo = inputs(0)
    assert np.isnan(var).any() and np.isposinf(var).any() and (var < 0).any()
    for flags, k in itertools.product((A, 0), (0, 6)):
        kw = dict(levels=8, want_levels=LEVELS, flags=flags, normal_power_log2=k, sigma_color=INF, sigma_plane=0.3)
        guided = g64.denoise_guided_f64(rgb, var, index, normal, point, albedo, var_floor=1e-4, **kw)
        plain = denoise_f64.denoise_f64(rgb, index, normal, point, albedo, **kw)
        for L in LEVELS:
            diff = np.abs(guided[L][0] - plain[L])
            assert np.isfinite(plain[L]).all() and (diff <= 2.0 ** -40 * np.abs(plain[L])).all(), (flags, k, L, float(diff.max()))


def test_the_variance_channel_alone_leaves_1225_16384_per_level():
    """§4.13: "with flat guides, wc = 1 and all 25 taps, W = 1 and V = v·Σh² = v·1225/16384".  33x31, flat guides, sigma_color = +inf, a
    noisy colour (which wc = 1 ignores) and one variance v everywhere: a pixel at least 2·(2^L − 1) from every border has read only
    such pixels at every level, so its variance after L levels is v·(1225/16384)^L — on the reference to REL_F64 per two levels, on
    the mirror within the reference's bound."""
    w, h = 33, 31
    index = np.zeros((h, w), np.int32)
    normal = np.zeros((h, w, 3), np.float32)
    normal[..., 2] = 1
    point = np.zeros((h, w, 3), np.float32)
    point[..., 0], point[..., 1] = np.meshgrid(np.arange(w), np.arange(h))
    rgb = np.random.default_rng(3331).random((h, w, 3)).astype(np.float32)
    var = np.empty((h, w, 3), np.float32)
    var[:] = (0.3, 0.2, 0.1)
    v = (float(var[0, 0, 0]) + float(var[0, 0, 1])) + float(var[0, 0, 2])
    kw = dict(flags=0, sigma_color=INF, sigma_plane=0.25, var_floor=1e-4, normal_power_log2=6)
    ref = g64.denoise_guided_f64(rgb, var, index, normal, point, levels=3, want_levels=(1, 2, 3), bound=True, **kw)
    mir = denoise_guided_ref.denoise(rgb, var, index, normal, point, None, levels=3, each_level=True, **kw)
    for L in (1, 2, 3):
        b = 2 * (2 ** L - 1)
        inner = (slice(b, h - b), slice(b, w - b))
        want = v * (1225 / 16384) ** L
        _, _, rv, vb, excluded = ref[L]
        assert rv[inner].size >= 15 and not excluded.any()
        assert (np.abs(rv[inner] - want) <= 2 * REL_F64 * want).all(), (L, float(np.abs(rv[inner] - want).max()), want)
        err = np.abs(mir[L - 1][1].astype(np.float64) - rv)
        assert (err <= vb).all(), (L, float((err / vb).max()))
        assert (np.abs(mir[L - 1][1][inner] - want) <= vb[inner] + 2 * REL_F64 * want).all(), L
        print(f"variance alone, L={L}: want {want:.9e}, reference off by {np.abs(rv[inner] - want).max() / want:.2e} relative, "
              f"mirror err/bound {float((err / vb).max()):.4f}")
