"""Temporal accumulation held to an f64 statement of its contract, without a GPU: tests/temporal_f64.py is the
section in numpy float64, written from its text and not from the mirror, with the projection solved from the camera's definition
(§4.10) and a derived per-value error bound.  Here the CPU restatement (tests/temporal_mirror.cpp) stays within that bound on
sequences that pan, move and turn a general camera with unequal spp; every listed misreading of the section, switched into the f64
reference, leaves the bound; the f64 reference gives the hand-derived rational answers; §4.15's statement of the projection's
accuracy holds at random points from 10 to 10^6 pixel widths away; and the orbit that tests/test_temporal_f64_gpu.py runs on the
device is run on the mirror with the oracle's G-buffer."""
import functools

import numpy as np
import pytest

import temporal_cases as cases
import temporal_f64
import temporal_ref
from rayz_amd import capi

SIZES = [(33, 9), (45, 23), (97, 41)]
PARAMS = {"defaults": {}, "binding": dict(alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)}
SEQUENCES = ("general", "moving", "moving-reset", "edge")


@functools.lru_cache(maxsize=None)
def frames_of(seq, w, h):
    make = {"general": cases.general_sequence, "moving": cases.moving_sequence, "moving-reset": cases.moving_sequence,
            "edge": cases.edge_sequence}[seq]
    return make(w, h, 5 * w + h)


def feed(handle, seq, w, h, prm, **kw):
    """The steps of a listed sequence through `handle`: a list of its per-step results."""
    frames = frames_of(seq, w, h)
    out = []
    for k, f in enumerate(frames):
        if seq == "moving-reset" and k == len(frames) - 1:
            handle.reset()
        out.append(handle.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], f.get("spp", 8), **prm, **kw))
    return out


@functools.lru_cache(maxsize=None)
def mirror_and_reference(seq, w, h, pname):
    """(mirror outputs, f64 reference outputs with bound and mask) per step; computed once and shared, never changed."""
    prm = PARAMS[pname]
    return feed(temporal_ref.Temporal(w, h), seq, w, h, prm), feed(temporal_f64.TemporalF64(w, h), seq, w, h, prm, bound=True)


@pytest.mark.parametrize("pname", list(PARAMS))
@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("seq", SEQUENCES)
def test_mirror_within_the_f64_bound(seq, w, h, pname):
    """Colour, variance and length of every step, at every non-excluded value; at most 2 % of a step's hit pixels excluded.  The
    moved steps blend (more than half of the hit pixels find history), except `edge`'s, whose point is the refused border."""
    got, ref = mirror_and_reference(seq, w, h, pname)
    frames = frames_of(seq, w, h)
    for k, (g, r, f) in enumerate(zip(got, ref, frames)):
        hit = f["index"] >= 0
        ratios, share = temporal_f64.within_bound(g, r, hit, f"{seq} {w}x{h} {pname} step {k}")
        found = float((g[2][hit] > f.get("spp", 8)).mean())
        print(f"{seq} {w}x{h} {pname} step {k}: |diff|/bound colour {ratios[0]:.3f} variance {ratios[1]:.3f} length {ratios[2]:.3f}; "
              f"excluded {share:.4f}; history found {found:.3f}")
        first = k == 0 or (seq == "moving-reset" and k == len(frames) - 1)
        assert found == 0 if first else (found > 0.5 or seq == "edge"), (seq, k, found)


def told_apart(misread, seq, w, h, pname):
    """The largest |mirror − misread reference| / bound-of-the-reference-as-written over the non-excluded values of a sequence, and
    where: (factor, step, output name, index)."""
    got, ref = mirror_and_reference(seq, w, h, pname)
    wrong = feed(temporal_f64.TemporalF64(w, h, misread=misread), seq, w, h, PARAMS[pname])
    best = (0.0, None, None, None)
    for k, (g, r, x) in enumerate(zip(got, ref, wrong)):
        bnds, ex = r[-2:]
        for name, gv, xv, b in zip(("colour", "variance", "length"), g, x, bnds):
            keep = ~ex if gv.ndim == 2 else np.broadcast_to(~ex[..., None], gv.shape)
            d = np.abs(gv.astype(np.float64) - xv)
            with np.errstate(all="ignore"):
                q = np.where(keep, np.where(d == 0, 0.0, d / b), 0.0)
            q = np.where(np.isnan(q), np.inf, q)  # (a NaN where the mirror is finite is as far out as a value gets)
            i = np.unravel_index(np.argmax(q), q.shape)
            if q[i] > best[0]:
                best = (float(q[i]), k, name, tuple(int(j) for j in i))
    return best


@pytest.mark.parametrize("misread", temporal_f64.MISREADINGS)
def test_every_misreading_leaves_the_bound(misread):
    """Each wrong reading of §4.15, switched into the f64 reference, differs from the mirror by more than the bound of the reference
    as written, on a non-excluded value of a listed sequence at 45x23 — the first sequence and parameter set that shows it is
    reported.  (A factor of inf: the reference says "no history" there, bound 0, and the misreading blends.)"""
    for seq in SEQUENCES:
        for pname in PARAMS:
            factor, k, name, at = told_apart(misread, seq, 45, 23, pname)
            if factor > 1:
                print(f"{misread}: leaves the bound by x{factor:.3g} on {seq} 45x23 {pname}, step {k}, {name} at {at}")
                return
    pytest.fail(f"{misread}: no listed sequence tells it from the contract")


def test_f64_reference_gives_the_hand_derived_answers():
    """Every case of tests/temporal_cases.py: the rational expectation lies within the f64 reference's own bound.  The pixels the
    cases put ON a decision's border by design (x = −1 exactly, γ = 0, B = 2^-6) are the ones the reference excludes — it cannot know
    the f32 run is exact there — and nothing else is."""
    on_a_border = {"shift-1-0": 4, "shift-2-0": 4, "shift-0-1": 5, "shift-0-2": 5, "shift-1-1": 8, "shift-2-2": 8, "shift-2-1": 8,
                   "behind-camera": 1, "weight-at-2^-6": 1}
    for case in cases.cases():
        h, w = case.steps[0].index.shape
        ref = case.run(temporal_f64.TemporalF64(w, h),
                       lambda m, s: m.step(s.rgb, s.var, s.index, s.normal, s.point, s.camera, s.spp, bound=True, **s.params))
        (c, v, N), (bc, bv, bN), ex = ref[:3], ref[3], ref[4]
        skipped = 0
        for p, (cw, vw, Nw) in case.want.items():
            if ex[p]:
                skipped += 1
                continue
            for ch in range(3):
                assert abs(c[p][ch] - float(cw[ch])) <= bc[p][ch], (case.name, p, "colour", ch, c[p][ch], float(cw[ch]), bc[p][ch])
                assert abs(v[p][ch] - float(vw[ch])) <= bv[p][ch], (case.name, p, "variance", ch, v[p][ch], float(vw[ch]), bv[p][ch])
            assert abs(N[p] - float(Nw)) <= bN[p], (case.name, p, "length", N[p], float(Nw), bN[p])
        assert skipped == on_a_border.get(case.name, 0), (case.name, skipped, np.argwhere(ex).tolist())
        assert skipped < len(case.want) or case.name == "weight-at-2^-6"  # (that case IS its one border pixel)


def claim_cameras():
    """General cameras, some far from the origin (where the rounding of `from` outweighs the three FMAs)."""
    cams = cases.moving_cameras(97, 41)[1:]
    for off in ((40.0, -25.0, 13.0), (700.0, 300.0, -500.0)):
        c = dict(cams[2])
        for k in ("look_from", "px_origin"):
            c[k] = tuple(np.array(c[k]) + np.array(off))
        cams.append(c)
    return cams


@pytest.mark.parametrize("k", range(6))
def test_the_projection_is_as_accurate_as_the_section_says(k):
    """§4.15's closing statement: with e_row = 2^-24·Σ_j |M_row,j|·(5|w_j| + |from_j|) — M's rounding, w's rounding, from's rounding seen
    through w, and the three roundings of the row — the f32 x of a step is within (e_0 + |x|·e_2) / (t − e_2) + 2^-24·|x| of the f64
    solve of the camera's definition, y likewise with e_1, wherever γ = t > 2·e_2.  20,000 random points per camera, pixel positions
    over the whole frame and its margin, hit distances log-uniform from 10 to 10^6 pixel widths; the f32 values come from the
    mirror's own step statements (temporal_mirror_project)."""
    cam = claim_cameras()[k]
    rng = np.random.default_rng(100 + k)
    lf, A = temporal_f64.camera_system(cam)
    n = 20000
    xy = rng.uniform((-1, -1), (97, 41), (n, 2))
    D = 10 ** rng.uniform(1, 6, n)
    a = A[:, 2]
    t = D * np.linalg.norm(A[:, 0]) / np.linalg.norm(a)
    P = (lf + t[:, None] * (a + xy[:, :1] * A[:, 0] + xy[:, 1:] * A[:, 1])).astype(np.float32)
    M, fr = temporal_ref.camera_matrix(cam)
    got = temporal_ref.project(P, M, fr).astype(np.float64)
    x, y, ga, dx, dy, dga = temporal_f64.project(lf, A, P.astype(np.float64))
    clear = ga > 2 * dga
    assert clear.mean() > 0.99
    slack = 1 + 2.0 ** -20  # second order
    ex, ey, eg = np.abs(got[:, 0] - x), np.abs(got[:, 1] - y), np.abs(got[:, 2] - ga)
    Mi = np.linalg.inv(A)
    former = 6 * 2.0 ** -24 * (np.linalg.norm(Mi[0]) + np.abs(x) * np.linalg.norm(Mi[2])) * np.linalg.norm(P - lf, axis=1) / ga
    print(f"camera {k}: largest error / bound: x {(ex / dx)[clear].max():.3f}, y {(ey / dy)[clear].max():.3f}, gamma {(eg / dga)[clear].max():.3f}; "
          f"largest error in pixels {ex[clear].max():.3g}; largest error / the section's former statement (not asserted): "
          f"{(ex / former)[clear].max():.3g}")
    assert (ex <= dx * slack)[clear].all() and (ey <= dy * slack)[clear].all() and (eg <= dga * slack)[clear].all()
    # the points are where they were put: P's own rounding to f32, at most 2^-24·|P_j| per component, is all that moves them
    Mi = np.abs(Mi)
    moved = 2.0 ** -24 * np.sum(np.abs(P.astype(np.float64)) * (Mi[0][None] + np.abs(x)[:, None] * Mi[2][None]), axis=1) / ga
    assert (np.abs(x - xy[:, 0]) <= 2 * moved + 1e-9).all()


# ---- the orbit of tests/test_temporal_f64_gpu.py, on the CPU ----------------------------------------------------------------------
def test_mirror_within_the_bound_under_an_orbit(oracle):
    """threeSpheres at 64x36 through `temporal_cases.orbit_views` (look_from and look_at both move: an orbit and a dolly, not a
    pan), cameras from the oracle's camera_init, the first-hit G-buffer from tests/query_reference.py, oracle frames of 8 spp with a
    seed per frame: the mirror's steps lie within the f64 reference's bound, under the exclusion cap, and the moved steps find
    history for more than half of the hit pixels.  The twin of the device test: if that one fails and this one does not, the
    device is wrong and not the contract."""
    import query_reference as qr
    from denoise_guided_cases import guided_variance
    from rayz_amd import tracer

    t = tracer.threeSpheres(64, seed=3)
    t.samples_per_px, t.max_bounces = 8, 8
    t.set_gpu(render_seed=17, chunk_spp=4, traversal=capi.TRAVERSAL_BVH, tmin=1e-3)
    sd, p = t.scene_desc(), t.params()
    w, h = p.width, p.height
    gx, gy = np.meshgrid(np.arange(w), np.arange(h))
    m, r = temporal_ref.Temporal(w, h), temporal_f64.TemporalF64(w, h)
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
        p.samples_per_px, p.chunk_spp, p.seed = 8, 4, 100 + k
        raw = oracle.render_b(sd, c, p)[0].astype(np.float32)
        args = (raw, guided_variance(raw, 40 + k), idx, normal, point, c, 8)
        got, ref = m.step(*args), r.step(*args, bound=True)
        hit = idx >= 0
        ratios, share = temporal_f64.within_bound(got, ref, hit, f"orbit step {k}")
        found = float((got[2][hit] > 8).mean())
        print(f"orbit step {k}: |diff|/bound {ratios[0]:.3f} {ratios[1]:.3f} {ratios[2]:.3f}; excluded {share:.4f}; history found {found:.3f}")
        assert hit.any() and (found > 0.5 if k else found == 0), (k, found)
        assert m.last_static == r.last_static == (k == 1)
