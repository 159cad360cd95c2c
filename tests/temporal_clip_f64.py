"""DESIGN.md §4.28 in numpy float64, written from the section's text (not from tests/temporal_clip_mirror.cpp) on top of
tests/temporal_moments_f64.py and tests/temporal_background_f64.py: vectorised over the frame, no FMA, no fixed order of
summation.  `TemporalClipMomentsF64` is a moments handle in VARIANCE mode.  By default the background is passed through (INPUT)
and it states the HIT pixels; a pixel with id < 0 is tests/temporal_moments_f64.py's.  With `background=True` it is a handle in
ACCUMULATE mode and states the BACKGROUND pixels alone, on top of `TemporalBackgroundMomentsF64`, which states nothing else either:
a tap of rule 1 is then accepted iff it lies inside the frame and its index is < 0 — a comparison of integers, no margin — and the
variance is §4.27 rule 3's.  The plain step's colour and length are this step's by §4.16 rule 1, and its variance is untouched
by §4.28.

How it is built.  The OFF step is linear in the gathered history: c_out = fma(al, c − h, h), so the reference runs the OFF
reference, takes from it the taps' h = H/B, al and the gather itself, computes §4.28 rules 1 and 2 on the current frame,
and states rules 3 and 4 afresh from hk and hq'; W2, N, the spatial estimate and the selections are the OFF reference's.  It then
replaces the colour and m2 records the OFF reference kept, with their bounds, so that the next step gathers the clipped history.

The bound (first order, u = 2^-24, carried from step to step and doubled where it is reported, as in the modules below).
  Neighbourhood: §4.16 step 4's sums and their bounds as tests/temporal_moments_f64.py states them — δmu, δd, δ(dp·S0), δvn.
  Square root: sd = sqrt(vn), one rounding; δsd <= min( sqrt(δvn), δvn / (2·sqrt(vn − δvn)) ) + u·sd — the first is
  |√a − √b| <= √|a − b|, which holds near zero where the derivative does not.  e = g·sd: δe <= g·δsd + u·e.  lo = mu − e, hi = mu + e:
  δlo <= δmu + δe + u·|lo|, δhi likewise.
  Clamp: hk = clamp(h, lo, hi) is 1-Lipschitz in each of h, lo and hi: δhk <= max(δh, δlo, δhi) — whichever side the device and
  the reference decide, so the clamp needs no exclusion.
  Blend: δc_out <= k·δhk + |c − hk|·δal + al·u·|c − hk| + u·|c_out|  (tests/temporal_f64.py's expression with hk for h).
  Moments shift: t = hq − h·h CANCELS — hq and h·h agree to the history's spread — so its bound is stated against the magnitudes
  before the cancellation: δt <= δhq + 2|h|·δh + u·h² + u·|t|; tp = max(t, 0) is 1-Lipschitz; hq' = hk·hk + tp:
  δhq' <= δt + 2|hk|·δhk + u·hk² + u·|hq'| on a clipped channel, δhq on another.  WHICH of the two a channel takes is a decision: at
  h = lo the two agree where t >= 0 (hk = h: h² + t = hq) and differ by −t where t < 0, so a channel whose h lies within
  2(δh + δlo) of lo (or of hi) carries in addition |hk² + tp − hq| evaluated both ways: 2|h|·2(δh + δbox) + max(−t, 0) + δt.
  m2_out = fma(al, c·c − hq', hq') and the temporal estimate: tests/temporal_moments_f64.py's expressions.
`excluded` adds to the OFF reference's mask the pixels that found history and have a 7x7 normal test inside its doubled margin —
which is also the only way the decision S0 >= min_taps can differ, S0 being a count — and, through the OFF reference's own rule,
the pixels whose taps read an excluded record.

`misread=` switches in ONE wrong reading of §4.28 (MISREADINGS; what each does is said where it is switched in)."""
import numpy as np

from temporal_background_f64 import TemporalBackgroundMomentsF64
from temporal_f64 import DEFAULTS, U, VCAP  # noqa: F401
from temporal_ref import camera_key
from temporal_moments_f64 import TemporalMomentsF64, clamp, within_bound  # noqa: F401  (within_bound: for the tests)
from temporal_moments_ref import MOMENTS_DEFAULTS

MISREADINGS = ("population_variance", "gamma_times_variance", "output_clipped", "current_colour_clipped", "neighbourhood_from_history",
               "centre_excluded", "no_index_test", "min_max_box", "m2_not_shifted", "clip_in_static_step", "length_reset_on_clip")
CLIP_DEFAULTS = {"gamma": 1.0, "min_taps": 4.0}


class TemporalClipMomentsF64:
    def __init__(self, width, height, gamma=None, min_taps=None, misread=None, background=False):
        assert misread is None or misread in MISREADINGS, misread
        self.width, self.height, self.misread, self.background = width, height, misread, background
        self.g = np.float64(np.float32(CLIP_DEFAULTS["gamma"] if gamma is None else gamma))
        self.mc = np.float64(np.float32(CLIP_DEFAULTS["min_taps"] if min_taps is None else min_taps))
        self.off = TemporalBackgroundMomentsF64(width, height) if background else TemporalMomentsF64(width, height)
        self.inner = self.off if background else self.off.inner  # who keeps the colour records and the taps
        self.clipped = np.zeros((height, width), bool)  # the last step's: any channel clipped
        self.last_found = np.zeros((height, width), bool)

    def _box(self, c, idx, n, cm):
        """§4.28 rules 1 and 2 up to lo and hi for every pixel: (enough, lo, hi, δbox, nnear)."""
        mis = lambda name: self.misread == name  # noqa: E731
        h, w = self.height, self.width
        pad = lambda a: np.pad(a, [(3, 3), (3, 3)] + [(0, 0)] * (a.ndim - 2), mode="constant")  # noqa: E731
        cp, npad, ip = pad(c), pad(n), pad(idx)
        inside_p = np.pad(np.ones((h, w), bool), 3, constant_values=False)
        S0, S1, S2, A1 = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w, 3))
        lo_m, hi_m = np.full((h, w, 3), np.inf), np.full((h, w, 3), -np.inf)
        nnear = np.zeros((h, w), bool)
        for j in range(-3, 4):
            for i in range(-3, 4):
                sl = (slice(3 + j, 3 + j + h), slice(3 + i, 3 + i + w))
                cq, nq, iq = cp[sl], npad[sl], ip[sl]
                centre = i == 0 and j == 0
                dn = np.sum(nq * n, axis=-1)
                same = inside_p[sl] if mis("no_index_test") else inside_p[sl] & (iq == idx)
                acc = same & (centre or (dn >= cm))
                if self.background:  # rule 1 for a pixel with id < 0 (the caller selects those): the misses inside the frame
                    same = acc = inside_p[sl] & (iq < 0)
                    dn = np.full((h, w), np.inf)  # (no normal test: nothing within a margin)
                if centre and mis("centre_excluded"):
                    acc = np.zeros((h, w), bool)
                if not centre:
                    nnear |= same & (np.abs(dn - cm) <= 2 * 3 * U * np.sum(np.abs(nq * n), axis=-1))
                a3 = acc[..., None]
                S0 += acc
                S1 += np.where(a3, cq, 0.0)
                S2 += np.where(a3, cq * cq, 0.0)
                A1 += np.where(a3, np.abs(cq), 0.0)
                lo_m, hi_m = np.where(a3, np.minimum(lo_m, cq), lo_m), np.where(a3, np.maximum(hi_m, cq), hi_m)
        with np.errstate(all="ignore"):
            N0 = S0[..., None]
            ES1, ES2 = (N0 - 1) * U * A1, N0 * U * S2
            mu = S1 / N0
            Emu = ES1 / N0 + U * np.abs(mu)
            a = S2 / N0
            Ea = ES2 / N0 + U * a
            mm = mu * mu
            Emm = 2 * np.abs(mu) * Emu + U * mm
            d = a - mm
            Ed = Ea + Emm + U * np.abs(d)
            dp = np.where(d > 0, d, 0.0)
            t1 = dp * N0
            Et1 = N0 * Ed + U * t1
            if mis("population_variance"):  # /S0 for /(S0 − 1)
                vn, Evn = dp, Ed
            else:
                vn = t1 / (N0 - 1)
                Evn = Et1 / (N0 - 1) + U * vn
            sd = np.sqrt(vn)
            Esd = np.minimum(np.sqrt(Evn), Evn / (2 * np.sqrt(np.maximum(vn - Evn, 1e-300)))) + U * sd
            if mis("gamma_times_variance"):  # g·vn for g·sd
                sd = vn
            e = self.g * sd
            Ee = self.g * Esd + U * e
            lo, hi = mu - e, mu + e
            Ebox = Emu + Ee + U * np.maximum(np.abs(lo), np.abs(hi))
            if mis("min_max_box"):
                lo, hi = lo_m, hi_m
        enough = S0 >= self.mc
        return enough, lo, hi, Ebox, nnear

    def step(self, rgb, index, normal, point, camera, spp, bound=False, **params):
        """Returns (colour, variance, length, W2) in float64; with bound=True two more entries: the four bounds and (excluded,
        variance_excluded), as tests/temporal_moments_f64.py's step."""
        assert not (bound and self.misread), "the bound belongs to the reference as written"
        mis = lambda name: self.misread == name  # noqa: E731
        prm = {**DEFAULTS, **MOMENTS_DEFAULTS, **params}
        cm, wm = np.float64(np.float32(prm["normal_cos_min"])), np.float64(np.float32(prm["w2_max"]))
        h, w = self.height, self.width
        off = self.off
        c = np.asarray(rgb, np.float64).reshape(h, w, 3)
        n = np.asarray(normal, np.float64).reshape(h, w, 3)
        idx = np.asarray(index).reshape(h, w).astype(np.int64)
        hit = idx < 0 if self.background else idx >= 0  # the pixels this handle states
        inner = self.inner
        had = inner.has_history
        static = had and camera_key(camera) == inner.key
        Hp, Sp = (dict(inner.hist), dict(off.state)) if had else (None, None)  # what this step gathers from
        c_o, v_o, N_o, W2_o, (bc, bv, bN, bW), (ex, vex) = off.step(rgb, index, normal, point, camera, spp, bound=True, **params)
        Ec, Ev, EW = bc / 2, bv / 2, bW / 2
        self.clipped = np.zeros((h, w), bool)
        self.last_found = np.zeros((h, w), bool)
        moving = had and (not static or mis("clip_in_static_step"))
        if moving:
            T = inner.taps
            has, al, da, g = T["has"] & hit, T["al"], T["da0"], T["gather"]
            self.last_found = has
            h3, a3, k3, da3 = has[..., None], al[..., None], (1.0 - al)[..., None], da[..., None]
            with np.errstate(all="ignore"):
                hc, Eh = g(Hp["c"], Hp["Ec"])
                hq, Ehq = g(Sp["m2"], Sp["Em2"])
                src = Hp["c"] if mis("neighbourhood_from_history") else c  # the history frame's colours under the current guides
                enough, lo, hi, Ebox, nnear = self._box(src, idx, n, cm)
                use = h3 & enough[..., None]
                x = c_o if mis("output_clipped") else (c if mis("current_colour_clipped") else hc)
                below, above = use & (x < lo), use & (x > hi)
                xk = np.where(below, lo, np.where(above, hi, x))
                cl = below | above
                if mis("output_clipped"):  # the blended output clipped instead of the history
                    hk, c_b = hc, xk
                elif mis("current_colour_clipped"):
                    hk, c_b = hc, a3 * (xk - hc) + hc
                else:
                    hk = xk
                    c_b = a3 * (c - hk) + hk
                Ehk = np.where(use, np.maximum(Eh, Ebox), Eh)
                Ec_b = k3 * Ehk + np.abs(c - hk) * da3 + a3 * U * np.abs(c - hk) + U * np.abs(c_b)
                # rule 4
                t = hq - hc * hc
                Et = Ehq + 2 * np.abs(hc) * Eh + U * hc * hc + U * np.abs(t)
                tp = np.where(t > 0, t, 0.0)
                shifted = hk * hk + tp
                Eshift = Et + 2 * np.abs(hk) * Ehk + U * hk * hk + U * np.abs(shifted)
                hq2 = hq if mis("m2_not_shifted") else np.where(cl, shifted, hq)
                margin = 2 * (Eh + Ebox)
                edge = use & ((np.abs(hc - lo) <= margin) | (np.abs(hc - hi) <= margin))
                Ehq2 = np.where(cl, Eshift, Ehq) + np.where(edge, 2 * np.abs(hc) * margin + np.maximum(-t, 0.0) + Et, 0.0)
                cc = c * c
                m2_b = a3 * (cc - hq2) + hq2
                Em2_b = k3 * Ehq2 + np.abs(cc - hq2) * da3 + a3 * (U * cc + U * np.abs(cc - hq2)) + U * np.abs(m2_b)
                # §4.16 step 3 from the clipped colour and m2
                e = m2_b - c_b * c_b
                Ee = Em2_b + 2 * np.abs(c_b) * Ec_b + U * c_b * c_b + U * np.abs(e)
                ep = np.where(e > 0, e, 0.0)
                W3, EW3 = W2_o[..., None], EW[..., None]
                num = ep * W3
                Enum = W3 * Ee + ep * EW3 + U * num
                den = 1.0 - W3
                Eden = EW3 + U * den
                q = num / den
                Evt = np.where(den - 2 * Eden > 0, (Enum + q * Eden) / (den - 2 * Eden) + U * q, np.inf)
                vt = clamp(q)
            temporal = h3 & ~(W2_o > wm)[..., None]  # (a hit pixel's other choice is the spatial estimate, the sky's is +0: the OFF reference's)
            c_o, Ec = np.where(h3, c_b, c_o), np.where(h3, Ec_b, Ec)
            v_o, Ev = np.where(temporal, vt, v_o), np.where(temporal, Evt, Ev)
            self.clipped = cl.any(axis=-1)
            if mis("length_reset_on_clip"):
                N_o = np.where(self.clipped, float(spp), N_o)
            more = has & nnear
            ex, vex = ex | more, vex | more
            # the records the next step gathers: the clipped colour and m2, their bounds, and who is excluded
            H = inner.hist
            H["c"], H["Ec"] = np.where(h3, c_b, H["c"]), np.where(h3, Ec_b, H["Ec"])
            H["N"] = np.where(has, N_o, H["N"])
            H["excluded"] = H["excluded"] | more
            off.state["m2"], off.state["Em2"] = np.where(h3, m2_b, off.state["m2"]), np.where(h3, Em2_b, off.state["Em2"])
        res = (c_o, v_o, N_o, W2_o)
        if bound:
            res += ((2 * Ec, 2 * Ev, bN, bW), (ex, vex))
        return res
