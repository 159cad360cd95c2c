"""Temporal accumulation's background mode held to its f64 statement for the steps the plain one did not reach, without a GPU
(DESIGN.md §4.27 rules 2 and 3 with §4.23): tests/temporal_background_f64.py states the plain step with per-pixel counts and the
moments step with one spp and with counts, background pixels only.  Here the CPU restatement (tests/temporal_background_mirror.cpp)
in ACCUMULATE mode stays within that bound on the sequences and sizes of the plain statement's test; the reference alone stays
under the exclusion cap, over the background, and reaches both sides of rule 3's selection; and every new misreading leaves the
bound.  (tests/test_temporal_background_cpu.py holds the plain scalar step and everything that is not an f64 statement.)"""
import functools

import numpy as np
import pytest

import temporal_background_f64 as f64
import temporal_background_ref as ref
import temporal_cases
import temporal_counts_f64 as counts_f64

SIZES = [(33, 9), (97, 41)]
SEQUENCES = ("general", "moving", "edge")
BINDING = dict(alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)
# Equal frames of 8 spp put W2 on 1/2, 1/3, ..: w2_max = 0.45 lies between the first two, so a sequence's second step answers +0
# (W2_out > wm) and its third the temporal estimate; the default 0.25 is the fourth equal frame's border and is met by none here.
PLAIN_PARAMS = {"defaults": {}, "binding": BINDING}
MOMENTS_PARAMS = {"defaults": {}, "w2max-0.45": dict(w2_max=0.45), "w2max-0.45-binding": dict(w2_max=0.45, **BINDING)}
KINDS = ("plain-counts", "moments", "moments-counts")


def params_of(kind):
    return PLAIN_PARAMS if kind == "plain-counts" else MOMENTS_PARAMS


@functools.lru_cache(maxsize=None)
def frames_of(seq, w, h, counts):
    """A listed sequence with "spp": its own (8 where it has none), or per-pixel counts with NaN inputs where the count is 0."""
    make = {"general": temporal_cases.general_sequence, "moving": temporal_cases.moving_sequence, "edge": temporal_cases.edge_sequence}[seq]
    frames = make(w, h, 5 * w + h)
    if counts:
        return [dict(f, spp=f["counts"]) for f in counts_f64.sparse(frames, 13 * w + h + len(seq))]
    return [dict(f, spp=f.get("spp", 8)) for f in frames]


def step(handle, f, moments, **kw):
    if moments:
        return handle.step(f["rgb"], f["index"], f["normal"], f["point"], f["camera"], f["spp"], **kw)
    return handle.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], f["spp"], **kw)


@functools.lru_cache(maxsize=None)
def reference(seq, w, h, kind, pname):
    """The f64 reference's per-step results with bounds and masks, and per step (passthrough, found history); computed once."""
    moments = kind != "plain-counts"
    r = (f64.TemporalBackgroundMomentsF64 if moments else f64.TemporalBackgroundF64)(w, h)
    out, seen = [], []
    for f in frames_of(seq, w, h, kind != "moments"):
        out.append(step(r, f, moments, bound=True, **params_of(kind)[pname]))
        seen.append((r.last_passthrough.copy(), r.taps["has"].copy() if r.taps else np.zeros((h, w), bool)))
    return out, seen


@functools.lru_cache(maxsize=None)
def mirror(seq, w, h, kind, pname):
    moments = kind != "plain-counts"
    m = (ref.TemporalMoments if moments else ref.Temporal)(w, h, "accumulate")
    return [step(m, f, moments, **params_of(kind)[pname]) for f in frames_of(seq, w, h, kind != "moments")]


ALL = [(k, p) for k in KINDS for p in params_of(k)]
IDS = [f"{k}-{p}" for k, p in ALL]


@pytest.mark.parametrize("kind,pname", ALL, ids=IDS)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("seq", SEQUENCES)
def test_mirror_within_the_f64_bound(seq, w, h, kind, pname):
    """Every output of every background pixel of every step within the bound — or, where the reference holds it by selection from
    the inputs, equal to it with NaN equal to NaN; at most 2 % of a step's background excluded."""
    got, (want, seen) = mirror(seq, w, h, kind, pname), reference(seq, w, h, kind, pname)
    for k, (g, r, s, f) in enumerate(zip(got, want, seen, frames_of(seq, w, h, kind != "moments"))):
        bg = f["index"] < 0
        what = f"{seq} {w}x{h} {kind} {pname} step {k}"
        ratios, shares, equal = counts_f64.within_bound(g, r, bg, what, s[0], region=bg)
        print(f"{what}: |diff|/bound " + " ".join(f"{n} {x:.3f}" for n, x in zip(f64.NAMES, ratios))
              + f"; excluded {shares[0]:.4f}, variance {shares[1]:.4f}; {equal} values by equality; history found {float(s[1][bg].mean()):.3f}")


@pytest.mark.parametrize("kind,pname", ALL, ids=IDS)
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("seq", SEQUENCES)
def test_the_reference_alone_stays_under_the_cap(seq, w, h, kind, pname):
    """No mirror here.  On the reference's own masks, over the background: at most 2 % of every step excluded, per mask; no NaN
    where a record holds samples; behind the first step more than half of the sampled background finds history (three in ten
    with counts, where two records in five hold no samples and are refused); a counts step keeps history at pixels without
    samples; and with w2_max = 0.45 a moments sequence answers both +0 for a short history and the temporal estimate."""
    want, seen = reference(seq, w, h, kind, pname)
    frames = frames_of(seq, w, h, kind != "moments")
    short = estimated = 0
    for k, (r, s, f) in enumerate(zip(want, seen, frames)):
        bg = f["index"] < 0
        what = f"{seq} {w}x{h} {kind} {pname} step {k}"
        masks = r[-1] if isinstance(r[-1], tuple) else (r[-1],)
        shares = [float(m[bg].mean()) for m in masks]
        assert all(not m[~bg].any() and x <= 0.02 for m, x in zip(masks, shares)), (what, shares)
        live = bg & (r[2] > 0)
        for x in tuple(r[:len(r) - 2]) + tuple(r[-2]):
            assert not (np.isnan(x) & (live if x.ndim == 2 else live[..., None])).any(), what
        n = np.broadcast_to(f["spp"], bg.shape)
        has = s[1]
        found = float(has[bg & (n > 0)].mean())
        kept = int((bg & has & (n == 0)).sum())
        print(f"{what}: excluded " + " ".join(f"{x:.4f}" for x in shares) + f"; history found {found:.3f}; kept without a sample {kept}")
        assert found == 0 if k == 0 else found > (0.5 if kind == "moments" else 0.3), (what, found)
        assert kind == "moments" or k == 0 or kept, what
        if kind != "plain-counts":
            W2 = r[3]
            wm = np.float32(MOMENTS_PARAMS[pname].get("w2_max", 0.25))
            short += int((bg & has & (W2 > wm)).sum())
            estimated += int((bg & has & ~(W2 > wm) & (r[1] > 0).any(axis=-1)).sum())
    if kind != "plain-counts" and pname != "defaults":
        assert short and estimated, (seq, kind, pname, short, estimated)


def told_apart(misread, seq, w, h, kind, pname):
    """The largest |mirror − misread reference| / bound-of-the-reference-as-written over the non-excluded background values of a
    sequence, and where: (factor, step, output name, index)."""
    moments = kind != "plain-counts"
    got, (want, _) = mirror(seq, w, h, kind, pname), reference(seq, w, h, kind, pname)
    wrong = (f64.TemporalBackgroundMomentsF64 if moments else f64.TemporalBackgroundF64)(w, h, misread=misread)
    best = (0.0, None, None, None)
    for k, (g, r, f) in enumerate(zip(got, want, frames_of(seq, w, h, kind != "moments"))):
        x = step(wrong, f, moments, **params_of(kind)[pname])
        bnds, masks = r[-2], (r[-1] if moments else (r[-1], r[-1]))
        for name, gv, xv, b in zip(f64.NAMES, g, x, bnds):
            use = ~(masks[1] if name == "variance" else masks[0]) & (f["index"] < 0)
            keep = use if gv.ndim == 2 else np.broadcast_to(use[..., None], gv.shape)
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


@pytest.mark.parametrize("misread", f64.COUNTS_MISREADINGS + f64.MOMENTS_MISREADINGS)
def test_every_new_misreading_leaves_the_bound(misread):
    """Each wrong reading of §4.27's counts and moments rules, switched into the f64 reference, differs from the mirror by more than
    the bound of the reference as written, on a non-excluded background value of a listed sequence at 97x41: the counts rules on the
    plain handle with counts, the variance's on the moments handle with one spp and, failing that, with counts."""
    kinds = ("plain-counts",) if misread in f64.COUNTS_MISREADINGS else ("moments", "moments-counts")
    for kind in kinds:
        for seq in SEQUENCES:
            for pname in params_of(kind):
                factor, k, name, at = told_apart(misread, seq, 97, 41, kind, pname)
                if factor > 1:
                    print(f"{misread}: leaves the bound by x{factor:.3g} on {seq} 97x41 {kind} {pname}, step {k}, {name} at {at}")
                    return
    pytest.fail(f"{misread}: no listed sequence tells it from the contract")


def test_uniform_counts_are_the_scalar_step():
    """The plain and the moments statement stepped with an array of one value equal themselves stepped with that scalar exactly:
    values, bounds and masks, on the moving sequence with every parameter binding."""
    w, h = 33, 9
    frames = temporal_cases.moving_sequence(w, h, 5 * w + h)
    for moments, prm in ((False, BINDING), (True, MOMENTS_PARAMS["w2max-0.45-binding"])):
        make = f64.TemporalBackgroundMomentsF64 if moments else f64.TemporalBackgroundF64
        a, b = make(w, h), make(w, h)
        for k, f in enumerate(frames):
            x = step(a, dict(f, spp=8), moments, bound=True, **prm)
            y = step(b, dict(f, spp=np.full((h, w), 8, np.int32)), moments, bound=True, **prm)
            flat = lambda r: [z for part in r for z in (flat(part) if isinstance(part, tuple) else [part])]  # noqa: E731
            for i, (p, q) in enumerate(zip(flat(x), flat(y))):
                assert np.array_equal(p, q, equal_nan=True), (moments, k, i)
