"""Temporal accumulation's counts step held to an f64 statement of its contract, without a GPU:
tests/temporal_counts_f64.py is the section in numpy float64, written from its text and not from the mirror, inside §4.15's and
§4.16's f64 statements, with a derived per-value error bound.  Here the CPU restatements (tests/temporal_counts_mirror.cpp, plain and
moments) stay within that bound under counts drawn per pixel with NaN inputs wherever the count is 0; the reference alone stays under
the exclusion cap and its inputs reach every rule; every listed misreading of the section, switched into the reference, leaves the
bound; an array of one count is the scalar step exactly; and the reference gives the hand-derived rational answers."""
import functools

import numpy as np
import pytest

import temporal_cases as cases
import temporal_counts_cases
import temporal_counts_f64 as f64
import temporal_counts_ref

SIZES = [(33, 9), (45, 23), (97, 41)]
BINDING = dict(alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)
PLAIN_PARAMS = {"defaults": {}, "binding": BINDING}
MOMENTS_PARAMS = {"w2max-half": dict(w2_max=0.5), "all-spatial-2-taps": dict(w2_max=0.0, min_taps=2.0), "all-temporal": dict(w2_max=1.0),
                  "w2max-half-binding": dict(w2_max=0.5, **BINDING)}
SEQUENCES = ("general", "moving", "moving-reset", "edge")


def params_of(moments):
    return MOMENTS_PARAMS if moments else PLAIN_PARAMS


@functools.lru_cache(maxsize=None)
def frames_of(seq, w, h):
    """A listed sequence with per-pixel counts and NaN inputs where the count is 0 (`temporal_counts_f64.sparse`)."""
    make = {"general": cases.general_sequence, "moving": cases.moving_sequence, "moving-reset": cases.moving_sequence,
            "edge": cases.edge_sequence}[seq]
    return f64.sparse(make(w, h, 5 * w + h), 11 * w + h + len(seq))


def step_args(f, moments, counts=None):
    counts = f["counts"] if counts is None else counts
    if moments:
        return f["rgb"], f["index"], f["normal"], f["point"], f["camera"], counts
    return f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], counts


def feed(handle, frames, seq, moments, prm, probe=None, **kw):
    """The steps of a listed sequence through `handle`: its per-step results and, per step, what `probe(handle)` returned."""
    out, seen = [], []
    for k, f in enumerate(frames):
        if seq == "moving-reset" and k == len(frames) - 1:
            handle.reset()
        out.append(handle.step(*step_args(f, moments), **prm, **kw))
        seen.append(probe(handle) if probe else None)
    return out, seen


def rules_met(r):
    """What the reference's last step says of its own pixels: (passthrough, found history, a tap with b > 0 refused by rule 1 alone,
    a length decision within its margin)."""
    inner = getattr(r, "inner", r)
    T = inner.taps
    had = inner.last_had
    z = np.zeros((r.height, r.width), bool)
    return (r.last_passthrough.copy(), T["has"].copy() if had else z, inner.refused_empty.copy() if had else z,
            inner.length_near.copy() if had else z)


@functools.lru_cache(maxsize=None)
def reference(seq, w, h, moments, pname):
    """The f64 reference's per-step results with bounds and masks, and `rules_met` per step; computed once, never changed."""
    make = f64.TemporalMomentsF64 if moments else f64.TemporalF64
    return feed(make(w, h), frames_of(seq, w, h), seq, moments, params_of(moments)[pname], probe=rules_met, bound=True)


@functools.lru_cache(maxsize=None)
def mirror(seq, w, h, moments, pname):
    make = temporal_counts_ref.TemporalMomentsCounts if moments else temporal_counts_ref.TemporalCounts
    return feed(make(w, h), frames_of(seq, w, h), seq, moments, params_of(moments)[pname])[0]


def report(what, ratios, shares, equal, extra=""):
    print(f"{what}: |diff|/bound " + " ".join(f"{n} {x:.3f}" for n, x in zip(f64.NAMES, ratios))
          + f"; excluded {shares[0]:.4f}, variance {shares[1]:.4f}; {equal} values by equality{extra}")


ALL = [(False, p) for p in PLAIN_PARAMS] + [(True, p) for p in MOMENTS_PARAMS]
IDS = [("moments-" if m else "plain-") + p for m, p in ALL]


@pytest.mark.parametrize("moments,pname", ALL, ids=IDS)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("seq", SEQUENCES)
def test_mirror_within_the_f64_bound(seq, w, h, moments, pname):
    """Every output of every step of the counts mirrors at every non-excluded value — within the bound, or, where the reference
    holds the value by selection from the inputs, equal to it with NaN equal to NaN; at most 2 % of a step's hit pixels excluded."""
    got, (ref, seen) = mirror(seq, w, h, moments, pname), reference(seq, w, h, moments, pname)
    for k, (g, r, s, f) in enumerate(zip(got, ref, seen, frames_of(seq, w, h))):
        what = f"{seq} {w}x{h} {IDS[ALL.index((moments, pname))]} step {k}"
        ratios, shares, equal = f64.within_bound(g, r, f["index"] >= 0, what, s[0])
        report(what, ratios, shares, equal)
        assert equal > 0, what  # (every frame has a background and unsampled pixels without history)


@pytest.mark.parametrize("moments,pname", ALL, ids=IDS)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("seq", SEQUENCES)
def test_the_reference_alone_stays_under_the_cap_and_meets_every_rule(seq, w, h, moments, pname):
    """No mirror here.  On the reference's own masks: at most 2 % of every step's hit pixels excluded, per mask; rule 1's margin
    never fires; no NaN at a pixel whose record holds samples; between 0.2 and 0.6 of the counts are 0; and each of the steps 2
    onward that reads history has hit pixels with n > 0 that blend, with n = 0 that keep their history, and with a tap of b > 0
    refused only for its record's length of 0."""
    ref, seen = reference(seq, w, h, moments, pname)
    frames = frames_of(seq, w, h)
    zero = float(np.mean([(f["counts"] == 0).mean() for f in frames]))
    assert 0.2 < zero < 0.6, zero
    for k, (r, s, f) in enumerate(zip(ref, seen, frames)):
        what = f"{seq} {w}x{h} {IDS[ALL.index((moments, pname))]} step {k}"
        hit = f["index"] >= 0
        masks = r[-1] if moments else (r[-1],)
        shares = [float(m[hit].mean()) for m in masks]
        passthrough, has, refused, length_near = s
        n = f["counts"]
        blended, kept, empty = (int((hit & has & c).sum()) for c in (n > 0, n == 0, refused))
        print(f"{what}: excluded " + " ".join(f"{x:.4f}" for x in shares) + f"; zero counts {float((n == 0).mean()):.3f}; hit pixels "
              f"{int(hit.sum())}: blended {blended}, kept without a sample {kept}, with a refused empty tap {empty}")
        assert all(not m[~hit].any() and x <= 0.02 for m, x in zip(masks, shares)), (what, shares)
        assert not length_near.any(), what
        f64.no_nan_where_sampled(r, what)
        for m in masks:
            assert m.dtype == bool
        if k >= 2 and not (seq == "moving-reset" and k == len(frames) - 1):
            assert blended and kept and empty, (what, blended, kept, empty)


def told_apart(misread, seq, w, h, moments, pname):
    """The largest |mirror − misread reference| / bound-of-the-reference-as-written over the non-excluded values of a sequence, and
    where: (factor, step, output name, index).  A value the reference holds by selection has bound 0: any difference is inf, and
    a NaN on one side only is a difference."""
    got, (ref, _) = mirror(seq, w, h, moments, pname), reference(seq, w, h, moments, pname)
    make = f64.TemporalMomentsF64 if moments else f64.TemporalF64
    wrong, _ = feed(make(w, h, misread=misread), frames_of(seq, w, h), seq, moments, params_of(moments)[pname])
    best = (0.0, None, None, None)
    for k, (g, r, x) in enumerate(zip(got, ref, wrong)):
        bnds, masks = (r[4], r[5]) if moments else (r[3], (r[4], r[4]))
        for name, gv, xv, b in zip(f64.NAMES, g, x, bnds):
            out = masks[1] if name == "variance" else masks[0]
            keep = ~out if gv.ndim == 2 else np.broadcast_to(~out[..., None], gv.shape)
            gv = gv.astype(np.float64)
            with np.errstate(all="ignore"):
                d = np.abs(gv - xv)
                q = np.where(d == 0, 0.0, d / b)
            q = np.where(np.isnan(gv) & np.isnan(xv), 0.0, np.where(np.isnan(q), np.inf, q))
            q = np.where(keep, q, 0.0)
            i = np.unravel_index(np.argmax(q), q.shape)
            if q[i] > best[0]:
                best = (float(q[i]), k, name, tuple(int(j) for j in i))
    return best


@pytest.mark.parametrize("misread", f64.COUNTS_MISREADINGS)
def test_every_misreading_leaves_the_bound(misread):
    """Each wrong reading of §4.23, switched into the f64 reference, differs from the mirror by more than the bound of the
    reference as written, on a non-excluded value of a listed sequence and parameter set at 45x23 (the plain handle for the plain
    rules, the moments handle for the moments'); the first that shows it is printed."""
    moments = misread in f64.MOMENTS_MISREADINGS
    for seq in SEQUENCES:
        for pname in params_of(moments):
            factor, k, name, at = told_apart(misread, seq, 45, 23, moments, pname)
            if factor > 1:
                print(f"{misread}: leaves the bound by x{factor:.3g} on {seq} 45x23 {pname}, step {k}, {name} at {at}")
                return
    pytest.fail(f"{misread}: no listed sequence tells it from the contract")


@pytest.mark.parametrize("moments", [False, True], ids=["plain", "moments"])
@pytest.mark.parametrize("spp", [1, 8])
def test_uniform_counts_are_the_scalar_step(moments, spp):
    """§4.23 (a): the reference stepped with an array of one value spp >= 1 equals the reference stepped with that scalar EXACTLY —
    values, bounds and masks — on the moving sequence with every parameter binding: the counts rules changed nothing else."""
    w, h = 45, 23
    frames = cases.moving_sequence(w, h, 5 * w + h)
    make = f64.TemporalMomentsF64 if moments else f64.TemporalF64
    prm = MOMENTS_PARAMS["w2max-half-binding"] if moments else BINDING
    a, b = make(w, h), make(w, h)
    for k, f in enumerate(frames):
        x = a.step(*step_args(f, moments, spp), bound=True, **prm)
        y = b.step(*step_args(f, moments, np.full((h, w), spp, np.int32)), bound=True, **prm)
        flat = lambda r: [z for part in r for z in (flat(part) if isinstance(part, tuple) else [part])]  # noqa: E731
        fx, fy = flat(x), flat(y)
        assert len(fx) == len(fy) == (10 if moments else 7)
        for i, (p, q) in enumerate(zip(fx, fy)):
            assert np.array_equal(p, q, equal_nan=True), (k, i)
        assert np.array_equal(a.last_passthrough, b.last_passthrough)


# The pixels of the hand cases that the reference excludes, by case name, with the reason — as tests/test_temporal_moments_f64_cpu.py's
# ON_A_BORDER.
ON_A_BORDER = {
    # W2_out = hW = 1/2 = w2_max exactly, by design, and δhW > 0: the reference cannot know that the f32 gather is exact (variance only)
    "moments-zero-keeps-m2-and-W2": 1,
}


def holds_the_case(case, out, passthrough, moments):
    vals, bnds, masks = (out[:4], out[4], out[5]) if moments else (out[:3], out[3], (out[4], out[4]))
    skipped = 0
    for p, want in case.want.items():
        skipped += bool(masks[1][p])
        for name, v, b, x in zip(f64.NAMES, vals, bnds, want):
            if (masks[1] if name == "variance" else masks[0])[p]:
                continue
            by_selection = passthrough[p] and not (moments and name == "variance")
            for got, bound, exact in zip(np.atleast_1d(v[p]), np.atleast_1d(b[p]), x if isinstance(x, tuple) else (x,)):
                assert abs(got - float(exact)) <= bound, (case.name, p, name, got, float(exact), bound)
                assert not by_selection or (bound == 0 and got == float(exact)), (case.name, p, name, got, float(exact), bound)
    assert skipped == ON_A_BORDER.get(case.name, 0), (case.name, skipped, np.argwhere(masks[1]).tolist())
    return skipped


def test_f64_reference_gives_the_hand_derived_answers():
    """Every case of tests/temporal_counts_cases.py, plain and moments: each rational expectation lies within the reference's own
    bound, and equals it — bound 0 — where the value is there by selection from the inputs."""
    for moments, cs in ((False, temporal_counts_cases.cases()), (True, temporal_counts_cases.moments_cases())):
        for case in cs:
            h, w = case.steps[0].index.shape
            r = (f64.TemporalMomentsF64 if moments else f64.TemporalF64)(w, h)
            if moments:
                out = case.run(r, lambda m, s: m.step(s.rgb, s.index, s.normal, s.point, s.camera, s.counts, bound=True, **s.params))
            else:
                out = case.run(r, lambda m, s: m.step(s.rgb, s.var, s.index, s.normal, s.point, s.camera, s.counts, bound=True, **s.params))
            n = holds_the_case(case, out, r.last_passthrough, moments)
            print(f"{case.name}: {len(case.want) - n} of {len(case.want)} pixels held, {n} on a border")
