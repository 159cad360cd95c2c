"""Temporal accumulation's moments mode and feedback held to an f64 statement of their contracts, without a GPU (DESIGN.md §4.16,
§4.17): tests/temporal_moments_f64.py is the two sections in numpy float64, written from their text and not from the mirrors, on
top of §4.15's f64 statement, with a derived per-value error bound.  Here the CPU restatements (tests/temporal_moments_mirror.cpp,
tests/temporal_feedback_mirror.cpp) stay within that bound — colour, variance, length and W2 — on sequences that pan, move and turn
a general camera with unequal spp, at parameter sets that put both estimates into one step; the inputs are shown to do that, on the
reference's own masks; every listed misreading of either section, switched into the reference, leaves the bound; the reference
gives the hand-derived rational answers; a feedback handle that is never fed back is a moments handle; and §4.16's remark on the
f32 cancellation floor is measured."""
import functools

import numpy as np
import pytest

import temporal_cases as cases
import temporal_feedback_cases
import temporal_feedback_ref
import temporal_moments_cases
import temporal_moments_f64 as f64
import temporal_moments_ref

SIZES = [(33, 9), (45, 23), (97, 41)]
BINDING = dict(alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)
PARAMS = {"defaults": {}, "w2max-half": dict(w2_max=0.5), "w2max-half-binding": dict(w2_max=0.5, **BINDING),
          "all-spatial-2-taps": dict(w2_max=0.0, min_taps=2.0), "all-temporal": dict(w2_max=1.0)}
SEQUENCES = ("general", "moving", "moving-reset", "edge")
# `general_sequence` and `edge_sequence` carry no spp.  Two equal frames would give W2 = 1/2 at their static step — w2_max = 0.5 itself,
# a border that excludes every pixel's variance; 8 after 12 samples give a0 = 0.4, the binding alpha_min, and 16 after 4 give Ns = 20,
# the binding n_max: so 8, 4, 12 (W2 = 5/9 at the static step, a0 = 1/2 or 3/4 at the moved one).
PLAIN_SPP = (8, 4, 12)


@functools.lru_cache(maxsize=None)
def frames_of(seq, w, h):
    make = {"general": cases.general_sequence, "moving": cases.moving_sequence, "moving-reset": cases.moving_sequence,
            "edge": cases.edge_sequence}[seq]
    return make(w, h, 5 * w + h)


def frame_args(f, k):
    return f["rgb"], f["index"], f["normal"], f["point"], f["camera"], f.get("spp", PLAIN_SPP[k % 3])


@functools.lru_cache(maxsize=None)
def feedback_image(seq, w, h, k):
    """The image fed back behind step k of a listed sequence: a seeded `synthetic` frame that depends on no step's output (so the
    reference and whatever it is compared with get the same f32 numbers), with a NaN in one hit pixel and a +inf in another."""
    from denoise_cases import synthetic

    img = synthetic(w, h, 1000 + 7 * w + h + 31 * k)[0].copy()
    hits = np.argwhere(frames_of(seq, w, h)[k]["index"] >= 0)
    (ay, ax), (by, bx) = hits[len(hits) // 3], hits[2 * len(hits) // 3]
    img[ay, ax, 1], img[by, bx, 2] = np.nan, np.inf
    return img


def feed(handle, seq, w, h, prm, fed=False, **kw):
    """The steps of a listed sequence through `handle`, with `feedback_image` behind every step if `fed`: (per-step results,
    per-step `last_spatial` where the handle has one)."""
    frames = frames_of(seq, w, h)
    out, took = [], []
    for k, f in enumerate(frames):
        if seq == "moving-reset" and k == len(frames) - 1:
            handle.reset()
        out.append(handle.step(*frame_args(f, k), **prm, **kw))
        took.append(getattr(handle, "last_spatial", None))
        if fed:
            handle.feedback(feedback_image(seq, w, h, k))
    return out, took


@functools.lru_cache(maxsize=None)
def reference(seq, w, h, pname, fed):
    """The f64 reference's per-step results with bounds and masks, and which estimate each pixel took; computed once, never changed."""
    return feed(f64.TemporalMomentsF64(w, h, feedback=fed), seq, w, h, PARAMS[pname], fed=fed, bound=True)


@functools.lru_cache(maxsize=None)
def mirror(seq, w, h, pname, fed):
    m = temporal_feedback_ref.TemporalFeedback(w, h) if fed else temporal_moments_ref.TemporalMoments(w, h)
    return feed(m, seq, w, h, PARAMS[pname], fed=fed)[0]


def hold(got, ref, frames, what):
    worst, shares = [0.0] * 4, [0.0, 0.0]
    for k, (g, r, f) in enumerate(zip(got, ref, frames)):
        ratios, sh = f64.within_bound(g, r, f["index"] >= 0, f"{what} step {k}")
        print(f"{what} step {k}: |diff|/bound " + " ".join(f"{n} {x:.3f}" for n, x in zip(f64.NAMES, ratios))
              + f"; excluded {sh[0]:.4f}, variance {sh[1]:.4f}")
        worst = [max(a, b) for a, b in zip(worst, ratios)]
        shares = [max(a, b) for a, b in zip(shares, sh)]
    return worst, shares


@pytest.mark.parametrize("fed", [False, True], ids=["moments", "feedback"])
@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("seq", SEQUENCES)
def test_mirror_within_the_f64_bound(seq, w, h, pname, fed):
    """Colour, variance, length and W2 of every step of the moments mirror — and of the feedback mirror with an image written
    behind every step — at every non-excluded value; at most 2 % of a step's hit pixels in either mask."""
    hold(mirror(seq, w, h, pname, fed), reference(seq, w, h, pname, fed)[0], frames_of(seq, w, h),
         f"{seq} {w}x{h} {pname} {'feedback' if fed else 'moments'}")


@pytest.mark.parametrize("pname", ["w2max-half", "w2max-half-binding"])
@pytest.mark.parametrize("w,h", SIZES)
def test_the_inputs_put_both_estimates_into_one_step(w, h, pname):
    """On the REFERENCE's own selection: with w2_max = 0.5 each of the steps 2-4 of `moving_sequence` has at least half of its hit
    pixels on the temporal estimate and at least 2 % on the spatial one; and at 97x41 some moved step has a 32x8 workgroup tile
    without a spatial pixel (the kernel skips its LDS staging) and a tile with both kinds."""
    frames = frames_of("moving", w, h)
    _, took = reference("moving", w, h, pname, False)
    none, both = 0, 0
    for k in (2, 3, 4):
        hit, sp = frames[k]["index"] >= 0, took[k]
        share = float(sp[hit].mean())
        print(f"moving {w}x{h} {pname} step {k}: temporal {1 - share:.4f} spatial {share:.4f} of {int(hit.sum())} hit pixels")
        assert 1 - share >= 0.5 and share >= 0.02, (k, share)
        for ty in range(0, h, 8):
            for tx in range(0, w, 32):
                th, ts = hit[ty:ty + 8, tx:tx + 32], sp[ty:ty + 8, tx:tx + 32]
                none += bool(th.any() and not ts.any())
                both += bool(ts.any() and (th & ~ts).any())
    print(f"moving {w}x{h} {pname}: tiles of steps 2-4 without a spatial pixel {none}, with both kinds {both}")
    if (w, h) == (97, 41):
        assert none >= 1 and both >= 1


def told_apart(misread, seq, w, h, pname, fed):
    """The largest |mirror − misread reference| / bound-of-the-reference-as-written over the non-excluded values of a sequence, and
    where: (factor, step, output name, index)."""
    got, (ref, _) = mirror(seq, w, h, pname, fed), reference(seq, w, h, pname, fed)
    wrong, _ = feed(f64.TemporalMomentsF64(w, h, feedback=fed, misread=misread), seq, w, h, PARAMS[pname], fed=fed)
    best = (0.0, None, None, None)
    for k, (g, r, x) in enumerate(zip(got, ref, wrong)):
        bnds, (ex, vex) = r[4], r[5]
        for name, gv, xv, b in zip(f64.NAMES, g, x, bnds):
            out = vex if name == "variance" else ex
            keep = ~out if gv.ndim == 2 else np.broadcast_to(~out[..., None], gv.shape)
            with np.errstate(all="ignore"):
                d = np.abs(gv.astype(np.float64) - xv)
                q = np.where(keep, np.where(d == 0, 0.0, d / b), 0.0)
            q = np.where(np.isnan(q), np.inf, q)  # (a NaN where the mirror is finite is as far out as a value gets)
            i = np.unravel_index(np.argmax(q), q.shape)
            if q[i] > best[0]:
                best = (float(q[i]), k, name, tuple(int(j) for j in i))
    return best


def first_that_shows(misread, fed):
    for seq in SEQUENCES:
        for pname in PARAMS:
            factor, k, name, at = told_apart(misread, seq, 45, 23, pname, fed)
            if factor > 1:
                print(f"{misread}: leaves the bound by x{factor:.3g} on {seq} 45x23 {pname}, step {k}, {name} at {at}")
                return
    pytest.fail(f"{misread}: no listed sequence tells it from the contract")


@pytest.mark.parametrize("misread", f64.MISREADINGS)
def test_every_misreading_leaves_the_bound(misread):
    """Each wrong reading of §4.16, switched into the f64 reference, differs from the moments mirror by more than the bound of the
    reference as written, on a non-excluded value of a listed sequence and parameter set at 45x23; the first that shows it is
    printed.  (A factor of inf: the reference's value is there by selection, bound 0.)"""
    first_that_shows(misread, False)


@pytest.mark.parametrize("misread", f64.FEEDBACK_MISREADINGS)
def test_every_misreading_of_the_feedback_leaves_the_bound(misread):
    """.. and each wrong reading of §4.17, against the feedback mirror with an image written behind every step."""
    first_that_shows(misread, True)


ON_A_BORDER = {
    # W2_out = 1/2 = w2_max exactly, by design: the reference cannot know that the f32 run is exact there (variance only)
    "static-two": 2, "half-shift": 3, "E-non-finite-feedback": 3,
    # .. and the same at the eight pixels with history; the ninth, (0, 0), has x = −1 exactly: §4.15's own border
    "D-pan-over-a-fed-back-ramp": 9}


def holds_the_case(case, out):
    (vals, bnds, (ex, vex)) = out[:4], out[4], out[5]
    skipped = 0
    for p, want in case.want.items():
        skipped += bool(vex[p])
        for name, v, b, x in zip(f64.NAMES, vals, bnds, want):
            if (vex if name == "variance" else ex)[p]:
                continue
            for got, bound, exact in zip(np.atleast_1d(v[p]), np.atleast_1d(b[p]), x if isinstance(x, tuple) else (x,)):
                assert abs(got - float(exact)) <= bound, (case.name, p, name, got, float(exact), bound)
    assert skipped == ON_A_BORDER.get(case.name, 0), (case.name, skipped, np.argwhere(vex).tolist())
    return skipped


def test_f64_reference_gives_the_hand_derived_answers():
    """Every case of tests/temporal_moments_cases.py and tests/temporal_feedback_cases.py: each rational expectation lies within the
    f64 reference's own bound — 0 where the value is there by selection: 2^32 for fewer than min_taps, 2^32 for 0/0, +0 on background
    — and the pixels the reference excludes are the ones ON_A_BORDER counts, which the cases put on a decision's border by design."""
    def step(m, s):
        return m.step(s.rgb, s.index, s.normal, s.point, s.camera, s.spp, bound=True, **s.params)

    for case in temporal_moments_cases.cases():
        h, w = case.steps[0].index.shape
        n = holds_the_case(case, case.run(f64.TemporalMomentsF64(w, h), step))
        print(f"{case.name}: {len(case.want) - n} of {len(case.want)} pixels held, {n} on a border")
    for case in temporal_feedback_cases.cases():
        h, w = case.steps[0].index.shape
        n = holds_the_case(case, case.run(f64.TemporalMomentsF64(w, h, feedback=True), step, lambda m, img: m.feedback(img)))
        print(f"{case.name}: {len(case.want) - n} of {len(case.want)} pixels held, {n} on a border")


@pytest.mark.parametrize("pname", ["defaults", "w2max-half-binding"])
def test_a_feedback_reference_that_is_never_fed_back_is_the_moments_reference(pname):
    """§4.17: "As long as no feedback is given m1 and the colour are the same numbers through the same operations" — values, bounds
    and masks of `TemporalMomentsF64(feedback=True)` equal those of `feedback=False` exactly."""
    a, _ = reference("moving", 45, 23, pname, False)
    b, _ = feed(f64.TemporalMomentsF64(45, 23, feedback=True), "moving", 45, 23, PARAMS[pname], bound=True)
    for k, (x, y) in enumerate(zip(a, b)):
        for p, q in zip(x[:4] + x[4] + x[5], y[:4] + y[4] + y[5]):
            assert np.array_equal(p, q, equal_nan=True), (k, pname)


@pytest.mark.parametrize("alpha_min", [0.0, 0.05])
def test_the_cancellation_floor_of_a_settled_pixel(alpha_min):
    """§4.16, "What the estimates are worth": 32 static frames through the mirror at w2_max = 1, colours between 0.9 and 1.1.
    First ONE constant frame, drawn once: the reference's e is exactly 0 from the second frame on, so its bound IS the floor of
    what the f32 step can be held to, and the mirror's vt must lie within it.  Then the same frame with every value moved by up to
    2^-12 of itself per frame — a true variance of the mean near 10^-10, far below the floor: what the mirror reports there is
    rounding, and must lie within the bound too.  (The first frame has 5 spp and the others 4: with equal frames a0 = 1/20 would
    meet alpha_min = 0.05 exactly at the twentieth, a border that excludes every pixel from then on.)  Printed: the largest vt of
    the mirror, the largest |vt − reference| and the largest bound."""
    w, h = 16, 8
    f = cases.plane_sequence(w, h, 5, [(0, 0)])[0]
    rng = np.random.default_rng(3)
    base = rng.uniform(0.9, 1.1, (h, w, 3))
    hit = f["index"] >= 0
    prm = dict(w2_max=1.0, alpha_min=alpha_min, n_max=float("inf"))
    for jitter in (0.0, 2.0 ** -12):
        m, r = temporal_moments_ref.TemporalMoments(w, h), f64.TemporalMomentsF64(w, h)
        for k in range(32):
            rgb = (base * (1 + jitter * rng.uniform(-1, 1, base.shape))).astype(np.float32)
            args = (rgb, f["index"], f["normal"], f["point"], f["camera"], 4 if k else 5)
            got, ref = m.step(*args, **prm), r.step(*args, bound=True, **prm)
            f64.within_bound(got, ref, hit, f"settled alpha_min {alpha_min} jitter {jitter} frame {k}")
        assert not ref[5][1].any() and (jitter or (ref[1][hit] == 0).all())
        vt, off, floor, W2 = got[1][hit].max(), np.abs(got[1] - ref[1])[hit].max(), ref[4][1][hit].max(), ref[3][hit].max()
        print(f"settled, alpha_min {alpha_min}, jitter {jitter:.1e}: after 32 frames W2 = {W2:.5f}; largest vt of the mirror {vt:.3e} "
              f"(of the reference {ref[1][hit].max():.3e}); largest |vt - reference| {off:.3e}; the reference's bound (the floor) {floor:.3e}")


# ---- the orbit of tests/test_temporal_moments_f64_gpu.py, on the CPU ------------------------------------------------------------
# Equal frames of 4 spp put W2 on 1/2, 1/3, 1/4, 1/5 to within rounding: w2_max = 0.5 would have every pixel of the static second frame
# on the selection's border, and the default 0.25 every pixel of the fourth.  So the orbit runs the defaults with w2_max moved off
# those values: 0.3 (the temporal estimate from the fourth frame on) and 0.45 (from the third).
ORBIT_PARAMS = {"w2max-0.3": dict(w2_max=0.3), "w2max-0.45": dict(w2_max=0.45)}


@pytest.mark.parametrize("pname", list(ORBIT_PARAMS))
def test_mirror_within_the_bound_under_an_orbit(oracle, pname):
    """threeSpheres at 64x36 through `temporal_cases.orbit_views`, cameras from the oracle's camera_init, the first-hit G-buffer
    from tests/query_reference.py, oracle frames of 4 spp in ONE chunk with a seed per frame — no variance input exists, the case
    the mode is for: the moments mirror's steps lie within the f64 reference's bound under both caps, and the moved steps find
    history for more than half of the hit pixels.  The twin of the device test."""
    import query_reference as qr
    from rayz_amd import capi, tracer

    t = tracer.threeSpheres(64, seed=3)
    t.samples_per_px, t.max_bounces = 4, 8
    t.set_gpu(render_seed=17, chunk_spp=4, traversal=capi.TRAVERSAL_BVH, tmin=1e-3)
    sd, p = t.scene_desc(), t.params()
    w, h = p.width, p.height
    gx, gy = np.meshgrid(np.arange(w), np.arange(h))
    m, r = temporal_moments_ref.TemporalMoments(w, h), f64.TemporalMomentsF64(w, h)
    for k, view in enumerate(cases.orbit_views()):
        c = cases.orbit_camera(oracle, view, w, h)
        lf, du, dv, po = (np.array(list(getattr(c, f))) for f in ("look_from", "px_du", "px_dv", "px_origin"))
        rays = np.zeros((h * w, 8))
        rays[:, 0:3], rays[:, 7] = lf, np.inf
        rays[:, 4:7] = (po[None, None] + gx[..., None] * du + gy[..., None] * dv - lf).reshape(-1, 3)
        rays = rays.astype(np.float32).astype(np.float64)
        idx, _, rec, _ = qr.brute_force(oracle, sd, rays, 1e-3, capi.PRECISION_F32)
        idx = idx.reshape(h, w).astype(np.int32)
        normal, point = (rec[:, a:a + 3].reshape(h, w, 3).astype(np.float32) for a in (5, 2))
        p.samples_per_px, p.chunk_spp, p.seed = 4, 4, 100 + k
        raw = oracle.render_b(sd, c, p)[0].astype(np.float32)
        args = (raw, idx, normal, point, c, 4)
        got, ref = m.step(*args, **ORBIT_PARAMS[pname]), r.step(*args, bound=True, **ORBIT_PARAMS[pname])
        hit = idx >= 0
        ratios, sh = f64.within_bound(got, ref, hit, f"orbit {pname} step {k}")
        found = float((got[2][hit] > 4).mean())
        print(f"orbit {pname} step {k}: |diff|/bound " + " ".join(f"{n} {x:.3f}" for n, x in zip(f64.NAMES, ratios))
              + f"; excluded {sh[0]:.4f}, variance {sh[1]:.4f}; history found {found:.3f}; spatial {float(r.last_spatial[hit].mean()):.3f}")
        assert hit.any() and (found > 0.5 if k else found == 0), (k, found)
        assert m.last_static == r.last_static == (k == 1)
