"""Temporal accumulation's background mode on the CPU: the restatement tests/temporal_background_mirror.cpp against
the hand-derived answers of tests/temporal_background_cases.py; in INPUT mode against the mirrors of the four existing steps, bit
for bit, outputs and history; in ACCUMULATE mode every pixel with id >= 0 against the INPUT-mode run, with the background
differing; the host's matrix for the exact cameras; and the interface's text."""
import functools
import os

import numpy as np
import pytest

import temporal_background_cases as cases
import temporal_background_f64 as f64
import temporal_background_ref as ref
import temporal_cases
import temporal_counts_ref
import temporal_moments_ref
import temporal_ref

SIZES = [(1, 1), (5, 3), (33, 9), (45, 23), (97, 41)]
ORIGINS = [(0, 0), (0, 0), (0.25, -0.625), (1.25, 0.375)]  # first, static, a fractional move, a move by (1, 1) from there
BINDING = dict(alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)
DRAW = np.array([0, 0, 1, 4, 8])
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} values differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}"


def sequences(w, h):
    """name -> frames, every frame with its "spp"."""
    out = {"plane": temporal_cases.plane_sequence(w, h, 100 * w + h, ORIGINS), "general": temporal_cases.general_sequence(w, h, 5 * w + h),
           "edge": temporal_cases.edge_sequence(w, h, 7 * w + h), "moving": temporal_cases.moving_sequence(w, h, 3 * w + h)}
    return {k: [dict(f, spp=f.get("spp", 8)) for f in v] for k, v in out.items()}


def sparse(frames, seed):
    """The frames with per-pixel counts from {0, 0, 1, 4, 8} for spp and NaN colour and variance wherever the count is 0."""
    rng = np.random.default_rng(seed)
    out = []
    for f in frames:
        counts = rng.choice(DRAW, size=f["index"].shape).astype(np.int32)
        rgb, var = f["rgb"].copy(), f["var"].copy()
        rgb[counts == 0] = np.nan
        var[counts == 0] = np.nan
        out.append(dict(f, rgb=rgb, var=var, spp=counts))
    return out


def plain(handle, f, **prm):
    return handle.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], f["spp"], **prm)


def moments(handle, f, **prm):
    return handle.step(f["rgb"], f["index"], f["normal"], f["point"], f["camera"], f["spp"], **prm)


def case_step(handle, s):
    handle.set_background(s.mode)
    if isinstance(handle, ref.Temporal):
        return handle.step(s.rgb, s.var, s.index, s.normal, s.point, s.camera, cases.counts_of(s), **s.params)
    return handle.step(s.rgb, s.index, s.normal, s.point, s.camera, cases.counts_of(s), **s.params)


@pytest.mark.parametrize("case", cases.cases(), ids=lambda c: c.name)
def test_mirror_gives_the_hand_derived_answers(case):
    h, w = case.steps[0].index.shape
    case.check(*case.run(ref.Temporal(w, h), case_step), "mirror")


@pytest.mark.parametrize("case", cases.moments_cases(), ids=lambda c: c.name)
def test_moments_mirror_gives_the_hand_derived_answers(case):
    h, w = case.steps[0].index.shape
    case.check(*case.run(ref.TemporalMoments(w, h), case_step), "mirror")


def test_the_exact_cameras_matrix():
    """For cam(ox', oy') then cam(ox, oy), G is exactly [[1, 0, ox - ox'], [0, 1, oy - oy'], [0, 0, 1]]; and for a move of look_from
    and px_origin by one vector it is the identity."""
    for (a, b), (c, d) in (((0, 0), (1, 0)), ((0.5, -2), (-1.25, 3)), ((-127 / 128, 0.25), (0, 0)), ((3, 1), (3, 1))):
        G = ref.background_matrix(temporal_cases.cam(a, b), temporal_cases.cam(c, d))
        assert G.tolist() == [1, 0, c - a, 0, 1, d - b, 0, 0, 1], G
    moved = dict(temporal_cases.cam(2, 1), look_from=(5.0, -3.0, -6.0), px_origin=(7.0, -2.0, 2.0))
    assert ref.background_matrix(temporal_cases.cam(2, 1), moved).tolist() == [1, 0, 0, 0, 1, 0, 0, 0, 1]


@pytest.mark.parametrize("w,h", SIZES)
def test_input_mode_is_the_existing_steps(w, h):
    """The new mirror in INPUT mode against tests/temporal_mirror.cpp, temporal_moments_mirror.cpp and temporal_counts_mirror.cpp:
    every output and every history record of every step, bit for bit, at the defaults and with the parameters binding."""
    for name, frames in sequences(w, h).items():
        for prm in ({}, BINDING):
            pairs = [(ref.Temporal(w, h), temporal_ref.Temporal(w, h), plain, frames),
                     (ref.TemporalMoments(w, h), temporal_moments_ref.TemporalMoments(w, h), moments, frames),
                     (ref.Temporal(w, h), temporal_counts_ref.TemporalCounts(w, h), plain, sparse(frames, w + h)),
                     (ref.TemporalMoments(w, h), temporal_counts_ref.TemporalMomentsCounts(w, h), moments, sparse(frames, w + h))]
            for mine, theirs, step, fs in pairs:
                for k, f in enumerate(fs):
                    for x, y in zip(step(mine, f, **prm), step(theirs, f, **prm)):
                        same_bits(x, y, f"{w}x{h} {name} {type(theirs).__name__} step {k} output")
                    for x, y in zip(mine.state(), theirs.state()):
                        same_bits(x, y, f"{w}x{h} {name} {type(theirs).__name__} step {k} history")


@pytest.mark.parametrize("w,h", SIZES)
def test_accumulate_mode_changes_the_background_only(w, h):
    """ACCUMULATE against INPUT on the same frames, all four steps: every pixel with id >= 0 has the same outputs and the same
    history record bit for bit; in every sequence at least one background pixel's output differs; and with counts no background
    pixel that found history keeps a NaN."""
    for name, frames in sequences(w, h).items():
        for make, step, fs, counts in ((ref.Temporal, plain, frames, False), (ref.TemporalMoments, moments, frames, False),
                                       (ref.Temporal, plain, sparse(frames, w + h), True),
                                       (ref.TemporalMoments, moments, sparse(frames, w + h), True)):
            a, b = make(w, h, "input"), make(w, h, "accumulate")
            differs = 0
            for k, f in enumerate(fs):
                hit = f["index"] >= 0
                ra, rb = step(a, f), step(b, f)
                for x, y in zip(ra, rb):
                    same_bits(x[hit], y[hit], f"{w}x{h} {name} {make.__name__} counts={counts} step {k} output on hit pixels")
                for x, y in zip(a.state(), b.state()):
                    same_bits(x[hit], y[hit], f"{w}x{h} {name} {make.__name__} counts={counts} step {k} history on hit pixels")
                differs += int((ra[0].view(np.uint32) != rb[0].view(np.uint32))[~hit].any())
                length = rb[2]
                if k and counts:  # a background pixel whose length grew beyond its own count found history: it holds no NaN
                    kept = ~hit & (length > f["spp"])
                    assert np.isfinite(rb[0][kept]).all() and np.isfinite(rb[1][kept]).all()
                assert (rb[2][~hit] >= ra[2][~hit]).all()
            if w * h > 1:  # (one pixel holds no background)
                bg_twice = any(((fs[k]["index"] < 0) & (fs[k + 1]["index"] < 0)).any() for k in range(len(fs) - 1))
                assert bg_twice, f"{w}x{h} {name}: no pixel is background in two consecutive frames"
                assert differs, f"{w}x{h} {name} {make.__name__} counts={counts}: no background pixel's output differs between the modes"


def test_the_mode_switches_mid_sequence():
    """INPUT, INPUT, ACCUMULATE, ACCUMULATE, INPUT over moving_sequence: each step equals the step of a handle that ran the same
    prefix and is in that step's mode — the mode is no state of the history."""
    w, h = 33, 9
    frames = sequences(w, h)["moving"]
    modes = ["input", "input", "accumulate", "accumulate", "input"]
    tm = ref.Temporal(w, h)
    for k, (f, mode) in enumerate(zip(frames, modes)):
        tm.set_background(mode)
        got = plain(tm, f)
        hit = f["index"] >= 0
        if mode == "input":
            same_bits(got[0][~hit], f["rgb"][~hit], f"step {k}: an INPUT step passes the background through")
            assert (got[2][~hit] == f["spp"]).all()
        elif k:
            assert (got[2][~hit] > f["spp"]).any(), f"step {k}: no background pixel found history"


# ---- the f64 statement (tests/temporal_background_f64.py) -------------------------------------------------------------------------
F64_SIZES = [(33, 9), (97, 41)]
F64_SEQUENCES = ("general", "moving", "edge")
F64_PARAMS = {"defaults": {}, "binding": BINDING}


@functools.lru_cache(maxsize=None)
def f64_frames(seq, w, h):
    make = {"general": temporal_cases.general_sequence, "moving": temporal_cases.moving_sequence, "edge": temporal_cases.edge_sequence}[seq]
    return [dict(f, spp=f.get("spp", 8)) for f in make(w, h, 5 * w + h)]


@functools.lru_cache(maxsize=None)
def mirror_and_reference(seq, w, h, pname):
    """(mirror outputs in ACCUMULATE mode, f64 reference outputs with bound and mask) per step; computed once, never changed."""
    prm = F64_PARAMS[pname]
    frames = f64_frames(seq, w, h)
    m, r = ref.Temporal(w, h, "accumulate"), f64.TemporalBackgroundF64(w, h)
    return [plain(m, f, **prm) for f in frames], [plain(r, f, bound=True, **prm) for f in frames]


@pytest.mark.parametrize("pname", list(F64_PARAMS))
@pytest.mark.parametrize("w,h", F64_SIZES)
@pytest.mark.parametrize("seq", F64_SEQUENCES)
def test_mirror_within_the_f64_bound(seq, w, h, pname):
    """Colour, variance and length of every background pixel of every step within the bound; at most 2 % of a step's background
    pixels excluded — the reference alone stays under the cap; the steps behind the first find history for the background."""
    got, want = mirror_and_reference(seq, w, h, pname)
    for k, (g, r, f) in enumerate(zip(got, want, f64_frames(seq, w, h))):
        bg = f["index"] < 0
        assert r[-1][bg].mean() <= 0.02, (seq, k, r[-1][bg].mean())
        ratios, share = f64.within_bound(g, r, bg, f"{seq} {w}x{h} {pname} step {k}")
        found = float((g[2][bg] > f["spp"]).mean())
        print(f"{seq} {w}x{h} {pname} step {k}: |diff|/bound colour {ratios[0]:.3f} variance {ratios[1]:.3f} length {ratios[2]:.3f}; "
              f"excluded {share:.4f}; history found {found:.3f}")
        assert found == 0 if k == 0 else found > 0.5, (seq, k, found)


@pytest.mark.parametrize("w,h", F64_SIZES)
@pytest.mark.parametrize("seq", F64_SEQUENCES)
def test_moments_colour_and_length_are_the_plain_steps(seq, w, h):
    """§4.16 rule 1 carries the bound to the moments step: its colour and length on background pixels are the plain step's bit for bit."""
    frames = f64_frames(seq, w, h)
    a, b = ref.Temporal(w, h, "accumulate"), ref.TemporalMoments(w, h, "accumulate")
    for k, f in enumerate(frames):
        bg = f["index"] < 0
        ra, rb = plain(a, f), moments(b, f)
        same_bits(ra[0][bg], rb[0][bg], f"{seq} {w}x{h} step {k} colour")
        same_bits(ra[2][bg], rb[2][bg], f"{seq} {w}x{h} step {k} length")


def told_apart(misread, seq, w, h, pname):
    """The largest |mirror − misread reference| / bound-of-the-reference-as-written over the non-excluded background values of a
    sequence, and where: (factor, step, output name, index)."""
    got, want = mirror_and_reference(seq, w, h, pname)
    wrong_handle = f64.TemporalBackgroundF64(w, h, misread=misread)
    frames = f64_frames(seq, w, h)
    best = (0.0, None, None, None)
    for k, (g, r, f) in enumerate(zip(got, want, frames)):
        x = plain(wrong_handle, f, **F64_PARAMS[pname])
        bnds, ex = r[-2:]
        use = ~ex & (f["index"] < 0)
        for name, gv, xv, b in zip(("colour", "variance", "length"), g, x, bnds):
            keep = use if gv.ndim == 2 else np.broadcast_to(use[..., None], gv.shape)
            d = np.abs(gv.astype(np.float64) - xv)
            with np.errstate(all="ignore"):
                q = np.where(keep, np.where(d == 0, 0.0, d / b), 0.0)
            q = np.where(np.isnan(q), np.inf, q)
            i = np.unravel_index(np.argmax(q), q.shape)
            if q[i] > best[0]:
                best = (float(q[i]), k, name, tuple(int(j) for j in i))
    return best


# the sequence each misreading is told apart on: the pans translate (so G's transpose and inverse, the half-pixel centres and the
# nearest tap show), moving_sequence moves look_from (the sky's false parallax) and mixes hits and misses among a pixel's taps
NAMED = {"history_left_at_input": "general", "G_transposed": "general", "G_inverted": "general", "sky_translated_with_look_from": "moving",
         "taps_accepted_whatever_index": "moving", "pixel_centres_at_half": "general", "refused_tap_in_B": "moving", "nearest_tap": "general"}


@pytest.mark.parametrize("misread", f64.MISREADINGS)
def test_every_misreading_leaves_the_bound(misread):
    """Each wrong reading of §4.27, switched into the f64 reference, differs from the mirror by more than the bound of the reference
    as written, on a non-excluded background value of its named sequence at 97x41."""
    factor, k, name, at = told_apart(misread, NAMED[misread], 97, 41, "defaults")
    print(f"{misread}: leaves the bound by x{factor:.3g} on {NAMED[misread]} 97x41, step {k}, {name} at {at}")
    assert factor > 1, (misread, factor)


def test_f64_reference_gives_the_hand_derived_answers():
    """Every plain case without counts: the rational expectation of a background pixel lies within the f64 reference's own bound,
    unless the case puts that pixel ON a decision's border by design (x' = width or -1 exactly, gamma = 0), where the reference
    excludes it."""
    for case in cases.cases():
        if any(hasattr(s, "counts") or s.mode != "accumulate" for s in case.steps):
            continue
        h, w = case.steps[0].index.shape
        out = case.run(f64.TemporalBackgroundF64(w, h),
                       lambda m, s: m.step(s.rgb, s.var, s.index, s.normal, s.point, s.camera, s.spp, bound=True, **s.params))
        (c, v, N), (bc, bv, bN), ex = out[:3], out[3], out[4]
        checked = 0
        for p, (cw, vw, Nw) in case.want.items():
            if ex[p] or case.steps[-1].index[p] >= 0:
                continue
            checked += 1
            for ch in range(3):
                assert abs(c[p][ch] - float(cw[ch])) <= bc[p][ch], (case.name, p, "colour", ch, c[p][ch], float(cw[ch]), bc[p][ch])
                assert abs(v[p][ch] - float(vw[ch])) <= bv[p][ch], (case.name, p, "variance", ch, v[p][ch], float(vw[ch]), bv[p][ch])
            assert abs(N[p] - float(Nw)) <= bN[p], (case.name, p, "length", N[p], float(Nw), bN[p])
        assert checked, case.name


def test_interface_text():
    """The header declares the constants and the two calls; the Python layer knows them."""
    from rayz_amd import capi

    text = open(os.path.join(ROOT, "include", "rayz_hip.h")).read()
    for s in ("#define RAYZ_TEMPORAL_BACKGROUND_INPUT      0u", "#define RAYZ_TEMPORAL_BACKGROUND_ACCUMULATE 1u",
              "int rayz_hip_temporal_set_background(RayzTemporal* tm, uint32_t mode);",
              "int rayz_hip_temporal_get_background(RayzTemporal* tm, uint32_t* mode);"):
        assert s in text, s
    assert capi.TEMPORAL_BACKGROUND == {"input": 0, "accumulate": 1}
    names = [n for n, _, _ in capi.PROTOTYPES]
    assert "rayz_hip_temporal_set_background" in names and "rayz_hip_temporal_get_background" in names
