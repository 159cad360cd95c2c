"""DESIGN.md §4.27 in numpy float64 — the plain step and, at the end, the moments step; each with one spp or with counts — written from the section's text (not from
tests/temporal_background_mirror.cpp): vectorised over the frame and the taps, no FMA, no fixed order of summation.  The
previous-frame position of a background pixel does not use §4.27's G at all: it comes from the camera's definition in §4.10 — the
centre ray of pixel (x, y) has the direction a + x·u + y·v with u = px_du, v = px_dv, a = px_origin − look_from, and the previous
frame's pixel (x', y') with the same direction solves [u' v' a']·(s·x', s·y', s) = a + x·u + y·v, by `numpy.linalg.solve` on the f64
camera fields.  look_from enters only through a and a'.

`TemporalBackgroundF64` is a handle in ACCUMULATE mode.  It states the BACKGROUND only: a background tap reads only records whose
index is < 0, which an earlier step of this rule wrote, so the records of hit pixels never reach a background pixel and are not
kept.  For a pixel with id >= 0 `step` returns the input with an infinite bound and never excludes it (tests/temporal_f64.py
states those; tests/test_temporal_background_cpu.py holds them to the INPUT-mode step bit for bit).  `step` has the signature of
`temporal_ref.Temporal.step`.  `misread=` switches in ONE wrong reading of §4.27 (MISREADINGS).

The error bound (first order, carried from step to step, DOUBLED where it is reported or used as a margin; u = 2^-24).

  Projection.  G is the f64 product of the previous camera's inverse and this camera's columns, each entry rounded to f32 once:
  δG_kj <= u|G_kj|.  xf = f32(px), yf = f32(py) are exact.  A row, α = fma(G_1, yf, fma(G_0, xf, G_2)), has two roundings, each at
  most u times a partial sum that Σ_j |G_kj||z_j| dominates, z = (x, y, 1).  Together

      δα <= 3u·Σ_j |G_kj||z_j| =: e_k        (k = 0, 1, 2 for α, β, γ)

  plus the f64 error of this module's solve and of the host's cross products, 16·2^-53·cond([u' v' a'])·Σ_j (|[u' v' a']^-1|·|[u v a]|)_kj|z_j|
  — against the magnitudes BEFORE the cancellation that leaves G: where the view did not turn, G is the identity up to entries of
  1e-15 that the two f64 computations do not share, and at x = 0 such an entry is all of α.  It is far below u for any sane camera
  but decides which taps lie within the margin of an integer position.  x' = α/γ is one rounded divide: δx <= (e_0 + |x'|·e_2)/(γ − e_2) + u|x'|, δy
  likewise — tests/temporal_f64.py's expression, as are the weights, the history, the blend and the continuity argument for
  integer positions (the 4×4 neighbourhood whose outer taps carry b = 0 and a δb near an integer): they are restated below
  unchanged.

`excluded`.  A background pixel of a step that reads history is excluded when one of its decisions lies within the doubled
propagated error of its border — γ > 0 (e_2); x' > −1, x' < W, y' > −1, y' < H (δx, δy); B >= 2^-6 (δB); a0 < am (δa0); Ns > nm (δNs) —
or when an accepted tap with b > 0 or δb > 0 reads a record that was excluded at the previous step.  A tap's own test, index < 0, is
a comparison of integers and has no margin.

Counts (`spp` an (h, w) integer array; §4.27 rules 2 and 3 with §4.23, whose f64 text is tests/temporal_counts_f64.py).  n = f32(count)
is exact.  A tap needs N_prev(q) > 0 as well — a refused tap adds nothing to B — and a pixel is `near` where a relevant tap has
0 < N_prev(q) <= 2·EN(q).  §4.23 rules 2-4 hold for a pixel with id < 0 and rule 5 is REPLACED: no history gives c_out = c,
v_out = clamp(s), N_out = n with bound 0 (a NaN input passes through and is compared by equality: `last_passthrough`); history
and n > 0 is the blend above with n per pixel; history and n = 0 keeps it by selection on the value — c_out = h (δh), v_out = hv
(δhv), N_out = hN > nm ? nm : hN (δhN), no a0 < am decision — so a NaN input reaches neither the outputs nor the records.  A static
step's one tap has b = 1 and B = 1: every mean is fma(1, x, 0) / 1 = x and the gather's rounding term is 0 (§4.23 (b)).

Moments: `TemporalBackgroundMomentsF64`, below.  COUNTS_MISREADINGS and MOMENTS_MISREADINGS are the wrong readings of these two:
zero_count_background_takes_input — rule 5 kept, a background pixel without samples passes its input through;
background_tap_ignores_length — a record of length 0 is accepted; background_variance_takes_spatial — where W2_out > wm the
background answers §4.16 step 4's estimate, which for a miss (normal zero: the centre alone, fewer than min_taps) is 2^32;
background_variance_zero_always — +0 as in the default mode; background_short_history_gets_vt — vt wherever history was found,
whatever W2_out."""
import numpy as np

from temporal_f64 import BMIN, U, VCAP, camera_system, within_bound  # noqa: F401  (within_bound: for the tests)
from temporal_ref import DEFAULTS, camera_key

MISREADINGS = ("history_left_at_input", "G_transposed", "G_inverted", "sky_translated_with_look_from", "taps_accepted_whatever_index",
               "pixel_centres_at_half", "refused_tap_in_B", "nearest_tap")
# .. of the counts steps and of the moments steps (below: "Counts", "Moments")
COUNTS_MISREADINGS = ("zero_count_background_takes_input", "background_tap_ignores_length")
MOMENTS_MISREADINGS = ("background_variance_takes_spatial", "background_variance_zero_always", "background_short_history_gets_vt")
NAMES = ("colour", "variance", "length", "W2")


class TemporalBackgroundF64:
    def __init__(self, width, height, misread=None):
        assert misread is None or misread in MISREADINGS + COUNTS_MISREADINGS + MOMENTS_MISREADINGS, misread
        self.width, self.height, self.misread = width, height, misread
        self.has_history = False
        self.key = self.cam = None
        self.hist = None  # dict: c, v (h, w, 3); N (h, w); id (h, w); Ec, Ev (h, w, 3); EN (h, w); excluded (h, w)
        self.taps = None  # what a step that rides the same taps needs (TemporalBackgroundMomentsF64)
        self.last_passthrough = None  # (h, w) bool: background pixels whose outputs the last step took from its inputs by selection

    def reset(self):
        self.has_history = False

    def step(self, rgb, var_rgb, index, normal, point, camera, spp, length=True, bound=False, **params):
        """Returns (colour (h, w, 3), variance (h, w, 3)[, length (h, w)]) in float64; with bound=True two more entries: the bounds
        (shaped like them; +inf on pixels with id >= 0) and the `excluded` mask (h, w)."""
        assert not (bound and self.misread), "the bound belongs to the reference as written"
        prm = {**DEFAULTS, **params}
        h, w = self.height, self.width
        f32 = lambda z: np.float64(np.float32(z))  # noqa: E731
        am, nm = f32(prm["alpha_min"]), f32(prm["n_max"])
        counts = np.ndim(spp) != 0
        if counts:
            spp = np.asarray(spp)
            assert spp.shape == (h, w) and spp.dtype.kind in "iu" and (spp >= 0).all() and (spp <= 2 ** 24).all(), (spp.shape, spp.dtype)
            spp = spp.astype(np.float64)  # n = f32(count), exact up to 2^24
        else:
            spp = float(spp)
        c = np.asarray(rgb, np.float64).reshape(h, w, 3)
        s = np.asarray(var_rgb, np.float64).reshape(h, w, 3)
        idx = np.asarray(index).reshape(h, w).astype(np.int64)
        with np.errstate(invalid="ignore"):
            s = np.where(~(s < VCAP), VCAP, np.where(s > 0, s, 0.0))
        lf, A = camera_system(camera)
        key = camera_key(camera)
        static = self.has_history and key == self.key
        bg = idx < 0
        has = np.zeros((h, w), bool)
        excluded = np.zeros((h, w), bool)
        c_out, v_out, N_out = c.copy(), s.copy(), (spp.copy() if counts else np.full((h, w), spp))
        self.taps = None
        Ec, Ev, EN = np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w))
        if self.has_history:
            with np.errstate(all="ignore"):
                has, excluded, (c_b, v_b, N_b), (Ec_b, Ev_b, EN_b) = self._blend(static, c, s, bg, lf, A, spp, am, nm, counts)
            sel = lambda m, a, b: np.where(m[..., None] if a.ndim == 3 else m, a, b)  # noqa: E731
            c_out, v_out, N_out = sel(has, c_b, c_out), sel(has, v_b, v_out), sel(has, N_b, N_out)
            Ec, Ev, EN = sel(has, Ec_b, Ec), sel(has, Ev_b, Ev), sel(has, EN_b, EN)
        self.hist = dict(c=c.copy() if self.misread == "history_left_at_input" else c_out, v=v_out, N=N_out, id=idx, Ec=Ec, Ev=Ev, EN=EN,
                         excluded=excluded)
        self.has_history, self.key, self.cam = True, key, (lf, A)
        self.last_passthrough = bg & ~has & ~excluded
        res = (c_out, v_out) + ((N_out,) if length else ())
        if bound:
            inf3, inf1 = np.where(bg[..., None], 0.0, np.inf), np.where(bg, 0.0, np.inf)
            res += ((2 * Ec + inf3, 2 * Ev + inf3) + ((2 * EN + inf1,) if length else ()), excluded)
        return res

    def _position(self, lf, A):
        """x', y', γ of every pixel centre in the previous frame and the bounds δx, δy, e_γ of the module docstring."""
        mis = self.misread
        h, w = self.height, self.width
        plf, pA = self.cam
        gy, gx = np.mgrid[0:h, 0:w]
        z = np.stack([gx, gy, np.ones((h, w))], axis=-1).reshape(-1, 3).astype(np.float64)
        if mis == "G_inverted":  # previous -> current
            sol = np.linalg.solve(A, pA @ z.T).T
        elif mis == "G_transposed":
            sol = z @ np.linalg.solve(pA, A)  # (G^T z)^T = z^T G
        elif mis == "sky_translated_with_look_from":  # the sky as points one ray parameter away, seen from the previous look_from
            sol = np.linalg.solve(pA, (A @ z.T) + (lf - plf)[:, None]).T
        else:
            sol = np.linalg.solve(pA, A @ z.T).T
        G = np.abs(np.linalg.solve(pA, A))
        load = np.abs(z) @ G.T
        own = np.abs(z) @ (np.abs(np.linalg.inv(pA)) @ np.abs(A)).T  # before the cancellation that leaves G: what f64 rounds against
        e = 3 * U * load + 16 * 2.0 ** -53 * np.linalg.cond(pA) * own
        ga = sol[:, 2]
        x, y = sol[:, 0] / ga, sol[:, 1] / ga
        den = np.where(ga - e[:, 2] > 0, ga - e[:, 2], np.nan)
        dx = (e[:, 0] + np.abs(x) * e[:, 2]) / den + U * np.abs(x)
        dy = (e[:, 1] + np.abs(y) * e[:, 2]) / den + U * np.abs(y)
        dx, dy = np.where(np.isnan(dx), np.inf, dx), np.where(np.isnan(dy), np.inf, dy)
        if mis == "pixel_centres_at_half":
            x, y = x - 0.5, y - 0.5
        return tuple(a.reshape(h, w) for a in (x, y, ga, dx, dy, e[:, 2]))

    # ---- rules 1-3 for a handle that has history -------------------------------------------------------------------------------
    def _blend(self, static, c, s, bg, lf, A, spp, am, nm, counts=False):
        mis = self.misread
        h, w = self.height, self.width
        H = self.hist
        gy, gx = np.mgrid[0:h, 0:w]
        near = np.zeros((h, w), bool)  # a decision within its margin
        if static:
            ok = bg.copy()
            qx, qy = gx[None], gy[None]
            b, db = np.ones((1, h, w)), np.zeros((1, h, w))
            inside = np.ones((1, h, w), bool)
        else:
            x, y, ga, dx, dy, dga = self._position(lf, A)
            ok = bg & (ga > 0) & (x > -1) & (x < w) & (y > -1) & (y < h)
            gnear = np.abs(ga) <= 2 * dga
            fnear = (ga > 0) & ((np.abs(x + 1) <= 2 * dx) | (np.abs(x - w) <= 2 * dx) | (np.abs(y + 1) <= 2 * dy) | (np.abs(y - h) <= 2 * dy))
            near |= bg & (gnear | fnear)
            x, y = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
            dx, dy = np.where(ok, dx, 0.0), np.where(ok, dy, 0.0)
            x0, y0 = np.floor(x), np.floor(y)
            off = np.arange(-1, 3, dtype=np.float64)
            def axis(t, t0, dt):  # noqa: E306
                dist = np.abs(t[None] - (t0[None] + off[:, None, None]))
                if mis == "nearest_tap":
                    return ((dist <= 0.5) & (np.cumsum(dist <= 0.5, axis=0) == 1)).astype(np.float64), np.zeros_like(dist)
                return np.maximum(0.0, 1.0 - dist), np.where(dist <= 1 + 2 * dt[None], dt[None] + 2 * U, 0.0)
            bx, dbx = axis(x, x0, dx)
            by, dby = axis(y, y0, dy)
            b = (by[:, None] * bx[None]).reshape(16, h, w)
            db = (by[:, None] * dbx[None] + dby[:, None] * bx[None] + dby[:, None] * dbx[None]).reshape(16, h, w) + U * b
            qx = (x0[None, None] + off[None, :, None, None] + 0 * off[:, None, None, None]).reshape(16, h, w).astype(np.int64)
            qy = (y0[None, None] + off[:, None, None, None] + 0 * off[None, :, None, None]).reshape(16, h, w).astype(np.int64)
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
        rel = (b > 0) | (db > 0)
        acc = inside & ok[None]
        if mis != "taps_accepted_whatever_index":
            acc = acc & (H["id"][qy, qx] < 0)
        if counts:
            # §4.27 rule 2 in a counts step: N_prev(q) > 0 as well (§4.23 rule 1), with the margin every decision has
            Nq = H["N"][qy, qx]
            near |= (acc & rel & (Nq > 0) & (Nq <= 2 * H["EN"][qy, qx])).any(axis=0)
            if mis != "background_tap_ignores_length":
                acc = acc & (Nq > 0)
        taint = (acc & rel & H["excluded"][qy, qx]).any(axis=0)
        ba = np.where(acc, b, 0.0)
        dba = np.where(acc, db, 0.0)
        B = np.sum(np.where(inside & ok[None], b, 0.0), axis=0) if mis == "refused_tap_in_B" else np.sum(ba, axis=0)
        dB = np.sum(dba, axis=0) + 3 * U * B
        near |= ok & (np.abs(B - BMIN) <= 2 * dB)
        has = ok & (B >= BMIN)
        div = np.where(has, B, 1.0)

        def gather(val, E):
            """h = Σ b v_q / B over accepted taps and its bound; val (h, w[, 3])."""
            ex = (lambda t: t[..., None]) if val.ndim == 3 else (lambda t: t)
            # the records are SELECTED before they meet a weight: a refused record may hold a NaN (§4.23), and 0·NaN is NaN
            vq, Eq = np.where(ex(acc), val[qy, qx], 0.0), np.where(ex(acc), E[qy, qx], 0.0)
            hh = np.sum(ex(ba) * vq, axis=0) / ex(div)
            Eh = (np.sum(ex(ba) * Eq, axis=0) + np.sum(ex(dba) * np.abs(vq - hh[None]), axis=0)
                  + rnd * np.sum(ex(ba) * np.abs(vq), axis=0)) / ex(div)
            return hh, Eh

        rnd = 0.0 if static else 8 * U  # (a static step's one tap has b = 1 and B = 1: every mean is fma(1, x, 0) / 1 = x, §4.23 (b))

        hc, Ehc = gather(H["c"], H["Ec"])
        hv, Ehv = gather(H["v"], H["Ev"])
        hN, EhN = gather(H["N"], H["EN"])
        Ns = hN + spp
        dNs = EhN + U * Ns
        a0 = spp / Ns
        da0 = a0 * dNs / Ns + U * a0
        al = np.where(a0 < am, am, a0)
        sampled = np.ones((h, w), bool)
        if counts:
            # §4.23 rule 4 on the background (§4.27 rule 3 replaces rule 5): found history and n = 0 — al = 0 by selection, no margin
            # on a0 < am, the input never read: c_out = h (δh), v_out = hv (δhv), N_out = hN > nm ? nm : hN (δhN)
            sampled = spp > 0
            dNs = np.where(sampled, dNs, EhN)
            al, da0 = np.where(sampled, al, 0.0), np.where(sampled, da0, 0.0)
        near |= has & (np.where(sampled, np.abs(a0 - am) <= 2 * da0, False) | (np.abs(Ns - nm) <= 2 * dNs))
        k = 1.0 - al
        a3, k3 = al[..., None], k[..., None]
        diff = c - hc
        c_b = a3 * diff + hc
        Ec = k3 * Ehc + np.abs(diff) * da0[..., None] + a3 * U * np.abs(diff) + U * np.abs(c_b)
        dk = da0 + U * k
        da2, dk2 = 2 * al * da0 + U * al * al, 2 * k * dk + U * k * k
        v_b = a3 * a3 * s + k3 * k3 * hv
        Ev = s * da2[..., None] + hv * dk2[..., None] + k3 * k3 * Ehv + U * k3 * k3 * hv + U * v_b
        N_b = np.where(Ns > nm, nm, Ns)
        if counts:
            kept = ~sampled[..., None]  # selected on the VALUE: the input of such a pixel may be a NaN
            if mis == "zero_count_background_takes_input":
                c_b, Ec, v_b, Ev = np.where(kept, c, c_b), np.where(kept, 0.0, Ec), np.where(kept, s, v_b), np.where(kept, 0.0, Ev)
            else:
                c_b, Ec, v_b, Ev = np.where(kept, hc, c_b), np.where(kept, Ehc, Ec), np.where(kept, hv, v_b), np.where(kept, Ehv, Ev)
        excluded = bg & (near | (has & taint))
        self.taps = dict(gather=gather, has=has, al=al, da0=da0, sampled=sampled)
        return has, excluded, (c_b, v_b, N_b), (Ec, Ev, dNs)


def clamp(t):
    """§4.16's clamp(t) = !(t < 2^32) ? 2^32 : (t > 0 ? t : 0): a NaN goes to 2^32."""
    with np.errstate(invalid="ignore"):
        return np.where(~(t < VCAP), VCAP, np.where(t > 0, t, 0.0))


class TemporalBackgroundMomentsF64(TemporalBackgroundF64):
    """§4.27 rule 3 for the moments step, background pixels only: m2 and W2 ride rule 2's taps (the plain statement's `taps`), then
    e, vt and the selection v_out = (found history AND !(W2_out > wm)) ? vt : +0.  There is no spatial estimate.  `step` has the
    signature of `temporal_moments_ref.TemporalMoments.step` and returns (colour, variance, length, W2); with bound=True two more
    entries, the four bounds (+inf on pixels with id >= 0) and (excluded, variance_excluded) — the second contains the first.

    The bounds are tests/temporal_moments_f64.py's, restated: hq = Q/B and hW = HW/B are the gather with E_m2 and E_W2; cc = c·c is
    one rounding; m2_out = fma(al, cc − hq, hq): δm2_out <= (1 − al)·δhq + |cc − hq|·δal + al·(u·cc + u·|cc − hq|) + u·|m2_out|;
    W2_out = fma(k·k, hW, al·al): δW2_out <= hW·δ(k·k) + k²·δhW + δ(al·al) + u·W2_out; e = m2_out − c_out·c_out:
    δe <= δm2_out + 2|c_out|·δc_out + u·c_out² + u·|e|; num = max(e, 0)·W2_out, den = 1 − W2_out, vt = clamp(num/den) with
    δvt <= (δnum + vt·δden) / (den − 2δden) + u·vt (no bound, inf, where den <= 2δden).  Without history m2_out = c·c (δ <= u·cc),
    W2_out = 1 and v_out = +0 by selection.  In a counts step a pixel with n = 0 that found history takes m2_out = hq (δhq) and
    W2_out = hW (δhW) by selection.  The VARIANCE of a pixel is excluded where the pixel is, and where it found history and W2_out
    lies within 2·δW2_out of wm with δW2_out > 0 — unless vt has no finite bound there, when nothing is held to it."""

    def __init__(self, width, height, misread=None):
        super().__init__(width, height, misread)
        self.state = None  # dict: m2, Em2 (h, w, 3); W2, EW (h, w)

    def step(self, rgb, index, normal, point, camera, spp, bound=False, **params):
        from temporal_moments_ref import MOMENTS_DEFAULTS

        assert not (bound and self.misread), "the bound belongs to the reference as written"
        mis = self.misread
        unknown = set(params) - set(DEFAULTS) - set(MOMENTS_DEFAULTS)
        assert not unknown, unknown
        wm = np.float64(np.float32({**MOMENTS_DEFAULTS, **params}["w2_max"]))
        plain = {k: v for k, v in params.items() if k in DEFAULTS}
        h, w = self.height, self.width
        c = np.asarray(rgb, np.float64).reshape(h, w, 3)
        bg = np.asarray(index).reshape(h, w) < 0
        had, S = self.has_history, self.state
        out = TemporalBackgroundF64.step(self, rgb, np.zeros((h, w, 3)), index, normal, point, camera, spp, bound=bound, **plain)
        c_out, N_out = out[0], out[2]
        if bound:
            (bc, _, bN), ex = out[3], out[4]
        else:
            bc, bN, ex = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w), bool)
        Ec = np.where(bg[..., None], bc, 0.0) / 2
        T = self.taps if had else None
        z3, z1 = np.zeros((h, w, 3)), np.zeros((h, w))
        cc = c * c
        has = T["has"] if had else np.zeros((h, w), bool)
        h3 = has[..., None]
        m2_o, Em2, W2_o, EW = cc, U * cc, np.ones((h, w)), z1
        with np.errstate(all="ignore"):
            if had:
                g, al, da = T["gather"], T["al"], T["da0"]
                k = 1.0 - al
                a3, k3, da3 = al[..., None], k[..., None], da[..., None]
                hq, Ehq = g(S["m2"], S["Em2"])
                hW, EhW = g(S["W2"], S["EW"])
                m2_b = a3 * (cc - hq) + hq
                Em2_b = k3 * Ehq + np.abs(cc - hq) * da3 + a3 * (U * cc + U * np.abs(cc - hq)) + U * np.abs(m2_b)
                dk = da + U * k
                da2, dk2 = 2 * al * da + U * al * al, 2 * k * dk + U * k * k
                W2_b = k * k * hW + al * al
                EW_b = hW * dk2 + k * k * EhW + da2 + U * W2_b
                kept = ~T["sampled"]  # a counts step's pixels with n = 0: selected on the VALUE, c may be a NaN
                m2_b, Em2_b = np.where(kept[..., None], hq, m2_b), np.where(kept[..., None], Ehq, Em2_b)
                W2_b, EW_b = np.where(kept, hW, W2_b), np.where(kept, EhW, EW_b)
                m2_o, Em2 = np.where(h3, m2_b, m2_o), np.where(h3, Em2_b, Em2)
                W2_o, EW = np.where(has, W2_b, W2_o), np.where(has, EW_b, EW)
            e = np.where(h3, m2_o - c_out * c_out, 0.0)
            Ee = np.where(h3, Em2 + 2 * np.abs(c_out) * Ec + U * c_out * c_out + U * np.abs(e), 0.0)
            ep = np.where(e > 0, e, 0.0)
            W3, EW3 = W2_o[..., None], EW[..., None]
            num = ep * W3
            Enum = W3 * Ee + ep * EW3 + U * num
            den = 1.0 - W3
            Eden = EW3 + U * den
            q = num / den
            Evt = np.where(den - 2 * Eden > 0, (Enum + q * Eden) / (den - 2 * Eden) + U * q, np.inf)
            vt = clamp(q)
        takes = has & ~(W2_o > wm)
        if mis == "background_short_history_gets_vt":
            takes = has
        t3 = takes[..., None]
        v_out, Ev = np.where(t3, vt, 0.0), np.where(t3, Evt, 0.0)
        if mis == "background_variance_zero_always":
            v_out = np.zeros((h, w, 3))
        if mis == "background_variance_takes_spatial":  # a miss's normal is zero: its 7x7 holds the centre alone, fewer than min_taps
            v_out = np.where((has & (W2_o > wm))[..., None], VCAP, v_out)
        v_out = np.where(bg[..., None], v_out, 0.0)
        wnear = bg & has & (EW > 0) & (np.abs(W2_o - wm) <= 2 * EW) & np.isfinite(np.where(t3, Evt, 0.0)).any(axis=-1)
        vex = ex | wnear
        keep = lambda a: np.where(bg[..., None] if a.ndim == 3 else bg, a, 0.0)  # noqa: E731  (only background records are ever read)
        self.state = dict(m2=keep(m2_o), Em2=keep(Em2), W2=keep(W2_o), EW=keep(EW))
        res = (c_out, v_out, N_out, np.where(bg, W2_o, 1.0))
        if bound:
            inf3, inf1 = np.where(bg[..., None], 0.0, np.inf), np.where(bg, 0.0, np.inf)
            res += ((bc, 2 * Ev + inf3, bN, 2 * EW + inf1), (ex, vex))
        return res
