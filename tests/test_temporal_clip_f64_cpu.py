"""The float64 statement of DESIGN.md §4.28 (tests/temporal_clip_f64.py) on the CPU: the mirror (tests/temporal_clip_mirror.cpp)
within its derived bound on the general, the moving and the edge sequence, at most 2 % of a step's hit pixels excluded, clipped and
unclipped pixels with history in every sequence; the plain step's colour and length equal to the moments step's bit for bit, which
carries the bound to it; and every named misreading outside the bound."""
import functools

import numpy as np
import pytest

import temporal_cases
import temporal_clip_f64 as f64
import temporal_clip_ref as ref

SIZES = [(33, 9), (97, 41)]
SEQUENCES = ("general", "moving", "edge")
PARAMS = {"defaults": {}, "w2_max 0.6": dict(w2_max=0.6)}  # (the second: the temporal estimate, which reads m2, from the second step on — 0.6 and
# not 1/2, which two equal frames reach exactly: every pixel would stand on the border of W2 > w2_max)
GAMMA = 1.0  # the default: chosen on the mirror so that every sequence has clipped and unclipped pixels with history (asserted below)


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    assert (a.view(np.uint32) == b.view(np.uint32)).all(), what


@functools.lru_cache(maxsize=None)
def frames_of(seq, w, h):
    make = {"general": temporal_cases.general_sequence, "moving": temporal_cases.moving_sequence, "edge": temporal_cases.edge_sequence}[seq]
    return [dict(f, spp=f.get("spp", 8)) for f in make(w, h, 5 * w + h)]


def step(handle, f, **kw):
    return handle.step(f["rgb"], f["index"], f["normal"], f["point"], f["camera"], f["spp"], **kw)


@functools.lru_cache(maxsize=None)
def mirror_and_reference(seq, w, h, pname="defaults"):
    """(mirror outputs, its clipped maps, f64 reference outputs with bounds and masks) per step; computed once, never changed."""
    frames, prm = frames_of(seq, w, h), PARAMS[pname]
    m, r = ref.TemporalMoments(w, h, clip="variance", gamma=GAMMA), f64.TemporalClipMomentsF64(w, h, gamma=GAMMA)
    got, maps = [], []
    for f in frames:
        got.append(step(m, f, **prm))
        maps.append(m.clipped.astype(bool))
    return got, maps, [step(r, f, bound=True, **prm) for f in frames]


@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("seq", SEQUENCES)
def test_mirror_within_the_f64_bound(seq, w, h, pname):
    got, maps, want = mirror_and_reference(seq, w, h, pname)
    some = none = 0
    for k, (g, cl, r, f) in enumerate(zip(got, maps, want, frames_of(seq, w, h))):
        hit = f["index"] >= 0
        ratios, shares = f64.within_bound(g, r, hit, f"{seq} {w}x{h} {pname} step {k}")  # (asserts the 2 % cap on both masks)
        found = hit & (g[2] > f["spp"])
        some, none = some + int(cl.sum()), none + int((found & ~cl).sum())
        print(f"{seq} {w}x{h} {pname} step {k}: |diff|/bound colour {ratios[0]:.3f} variance {ratios[1]:.3f} length {ratios[2]:.3f} W2 {ratios[3]:.3f}; "
              f"excluded {shares[0]:.4f} (variance {shares[1]:.4f}); of pixels with history clipped {cl.sum() / max(found.sum(), 1):.3f}")
    if w * h > 1000:
        assert some and none, (seq, some, none)


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("seq", SEQUENCES)
def test_plain_colour_and_length_are_the_moments_steps(seq, w, h):
    """§4.16 rule 1 carries the bound to the plain clip step: colour, length and map equal bit for bit; §4.28 leaves its variance alone."""
    a, b = ref.Temporal(w, h, clip="variance", gamma=GAMMA), ref.TemporalMoments(w, h, clip="variance", gamma=GAMMA)
    for k, f in enumerate(frames_of(seq, w, h)):
        ra = a.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], f["spp"])
        rb = step(b, f)
        same_bits(ra[0], rb[0], f"{seq} step {k} colour")
        same_bits(ra[2], rb[2], f"{seq} step {k} length")
        assert (a.clipped == b.clipped).all()


@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("seq", SEQUENCES)
def test_mirror_within_the_f64_bound_on_the_sky(seq, w, h, pname):
    """The same for the background pixels of a handle in ACCUMULATE mode (§4.28 rule 1's second kind of tap, §4.27 rule 3's variance)."""
    prm = PARAMS[pname]
    m = ref.TemporalMoments(w, h, "accumulate", clip="variance", gamma=GAMMA)
    r = f64.TemporalClipMomentsF64(w, h, gamma=GAMMA, background=True)
    some = none = 0
    for k, f in enumerate(frames_of(seq, w, h)):
        g, want = step(m, f, **prm), step(r, f, bound=True, **prm)
        bg = f["index"] < 0
        ratios, shares = f64.within_bound(g, want, bg, f"sky {seq} {w}x{h} {pname} step {k}")
        cl, found = m.clipped.astype(bool) & bg, bg & (g[2] > f["spp"])
        some, none = some + int(cl.sum()), none + int((found & ~cl).sum())
        print(f"sky {seq} {w}x{h} {pname} step {k}: |diff|/bound colour {ratios[0]:.3f} variance {ratios[1]:.3f} length {ratios[2]:.3f} W2 {ratios[3]:.3f}; "
              f"excluded {shares[0]:.4f} (variance {shares[1]:.4f}); of sky pixels with history clipped {cl.sum() / max(found.sum(), 1):.3f}")
    if w * h > 1000:
        assert some and none, (seq, some, none)


def told_apart(misread, seq, w, h, pname="defaults"):
    """The largest |mirror − misread reference| / bound-of-the-reference-as-written over the non-excluded hit values of a sequence."""
    got, _, want = mirror_and_reference(seq, w, h, pname)
    wrong = f64.TemporalClipMomentsF64(w, h, gamma=GAMMA, misread=misread)
    best = (0.0, None, None)
    for k, (g, r, f) in enumerate(zip(got, want, frames_of(seq, w, h))):
        x = step(wrong, f, **PARAMS[pname])
        bnds, (ex, vex) = r[4], r[5]
        hit = f["index"] >= 0
        for name, gv, xv, b in zip(("colour", "variance", "length", "W2"), g, x, bnds):
            use = hit & ~(vex if name == "variance" else ex)
            keep = use if gv.ndim == 2 else np.broadcast_to(use[..., None], gv.shape)
            d = np.abs(gv.astype(np.float64) - xv)
            with np.errstate(all="ignore"):
                q = np.where(keep, np.where(d == 0, 0.0, d / b), 0.0)
            q = np.where(np.isnan(q), np.inf, q)
            if q.max() > best[0]:
                best = (float(q.max()), k, name)
    return best


# the sequence each misreading is told apart on: general_sequence has the static step
# (m2 reaches an output only through the temporal estimate: w2_max = 0.6 selects it from the second step on)
NAMED = {m: ("moving", "defaults") for m in f64.MISREADINGS}
NAMED["clip_in_static_step"] = ("general", "defaults")
NAMED["m2_not_shifted"] = ("moving", "w2_max 0.6")


@pytest.mark.parametrize("misread", f64.MISREADINGS)
def test_every_misreading_leaves_the_bound(misread):
    factor, k, name = told_apart(misread, NAMED[misread][0], 97, 41, NAMED[misread][1])
    print(f"{misread}: leaves the bound by x{factor:.3g} on {' '.join(NAMED[misread])} 97x41, step {k}, {name}")
    assert factor > 1, (misread, factor)
