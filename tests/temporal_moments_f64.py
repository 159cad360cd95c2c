"""DESIGN.md §4.16 (moments mode) and §4.17 (feedback of the filtered colour) in numpy float64, written from the sections' text and
not from tests/temporal_moments_mirror.cpp, tests/temporal_feedback_mirror.cpp or the kernel headers: vectorised over the frame and
the taps, dots by `np.sum`, no FMA, no fixed order of summation, state kept in f64.  Everything §4.16 calls "§4.15's UNCHANGED" — the
projection solved from §4.10's camera, the taps, their acceptance, `B`, `al`, `k`, the static rule, colour and length — IS §4.15's
f64 statement: `TemporalMomentsF64` holds a `temporal_f64.TemporalF64`, steps it with a zero variance input, takes colour, length,
their bounds and the `excluded` mask from it, and reads the per-tap quantities it hands out (`TemporalF64.taps`: the accepted weights
`ba` and their bounds `dba`, the tap positions, `B`, `has`, `al`, `δa0`, and its `gather`, which is `h = Σ b v_q / B` with §4.15's
`δh`).  The state added here: `m2` (h, w, 3), `W2` (h, w) and, on a feedback handle, `m1` (h, w, 3), each with its carried bound.
`feedback(rgb)` is §4.17's write: finite pixels replace the colour of the side the last step wrote — which is the inner
reference's colour history, whose bound becomes 0 there, the image being the same f32 numbers in both runs — and nothing else.

`misread=` switches in ONE wrong reading of §4.16 (MISREADINGS) or, on a feedback handle, of §4.17 (FEEDBACK_MISREADINGS).  `step`
takes `spp` as one number or as an (h, w) integer array, the counts step of §4.23: the inner reference gets the array, m2 and W2 are
kept by selection where a pixel without samples found history, and step 4's neighbourhood runs over sampled positions
(tests/temporal_counts_f64.py has the text, the bounds and the wrong readings, COUNTS_MISREADINGS).

The error bound (first order, carried from step to step, DOUBLED where it is reported or used as a margin; u = 2^-24; δq = |q' − q|
for the f32 contract's q').  The input colour c and the guides are the same f32 numbers in both runs.  From tests/temporal_f64.py:
δc_out (its E_c), δal <= δa0, and for any history record v with carried bound E the gather

      δ(V/B) <= Σ b_q E_q / B + Σ δb_q |v_q − V/B| / B + 8u·Σ b_q |v_q| / B                              (§4.15's δh with the record's own E)

  Moments.  hq = Q/B, hW = HW/B, h1 = M1/B: the gather above with E_m2, E_W2, E_m1.  cc = c·c is one rounding: δcc <= u·cc.
  m2_out = fma(al, cc − hq, hq) = al·cc + (1 − al)·hq with the difference rounded first:
      δm2_out <= (1 − al)·δhq + |cc − hq|·δal + al·(u·cc + u·|cc − hq|) + u·|m2_out|
  m1_out = fma(al, c − h1, h1) is the colour's blend: δm1_out <= (1 − al)·δh1 + |c − h1|·δal + al·u·|c − h1| + u·|m1_out|.
  k = 1 − al: δk <= δal + u·k;  δ(k·k) <= 2k·δk + u·k²;  δ(al·al) <= 2al·δal + u·al²;  W2_out = fma(k·k, hW, al·al):
      δW2_out <= hW·δ(k·k) + k²·δhW + δ(al·al) + u·W2_out
  A pixel without history takes m2_out = c·c (δ <= u·cc: the product is rounded in f32 and exact here), m1_out = c and W2_out = 1
  by selection: bound 0 for the last two.

  Temporal estimate, with m = c_out (m1_out on a feedback handle) and δm its bound.  e = m2_out − (m·m), one product and one
  subtraction:  δe <= δm2_out + 2|m|·δm + u·m² + u·|e|.  Without history e = cc − cc = 0 EXACTLY in both runs (the same rounded
  product is subtracted from itself): bound 0, by selection.  ep = max(e, 0) is 1-Lipschitz: δep <= δe, nothing excluded.
      num = ep·W2_out:    δnum <= W2_out·δep + ep·δW2_out + u·num
      den = 1 − W2_out:   δden <= δW2_out + u·den
      vt = num / den:     δvt <= (δnum + vt·δden) / (den − 2δden) + u·vt       (the far end of the mean-value interval; den <= 2δden: no bound, inf)
  and the clamp is 1-Lipschitz and the identity at its own border.  Without history vt = clamp(0/0) = 2^32, bound 0.  Where e = 0
  with history the bound does not vanish: δvt >= (u·m² + δm2_out + ..)·W2/(1 − W2) — THAT is the f32 cancellation floor of the estimate.

  Spatial estimate.  The taps' colours are inputs (exact); S0 is a count (exact once the acceptances agree).  S1 takes S0 − 1
  rounded additions (the first, to +0, is exact), each of a partial sum of magnitude <= Σ|c_q|; S2 takes S0 FMAs, each rounding a
  partial sum <= Σ c_q²:   δS1 <= (S0 − 1)·u·Σ|c_q| <= 48u·Σ|c_q|,   δS2 <= S0·u·Σ c_q² <= 49u·Σ c_q².
      mu = S1/S0:  δmu <= δS1/S0 + u·|mu|;      a = S2/S0:  δa <= δS2/S0 + u·a;      mm = mu·mu:  δmm <= 2|mu|·δmu + u·mu²
      d = a − mm:  δd <= δa + δmm + u·|d|;      dp = max(d, 0):  δdp <= δd
      t1 = dp·S0:  δt1 <= S0·δd + u·t1;         t2 = t1/(S0 − 1):  δt2 <= δt1/(S0 − 1) + u·t2
      vs = t2·W2_out:  δvs <= W2_out·δt2 + t2·δW2_out + u·vs,   then the clamp.
  S0 < mt: vs = 2^32 by selection, bound 0.  Background: v_out = +0 by selection, bound 0.

What is dropped is second order, so the reported bounds are 2·E and every decision margin is 2·(its δ).

Exclusions (bound=True returns two masks).  `excluded` is §4.15's, taint included: colour, length and W2 of a pixel are excluded
exactly there — m2, W2 and m1 ride the same taps.  The VARIANCE of a pixel is excluded there and, besides, (a) where W2_out lies
within 2·δW2_out of wm and δW2_out > 0 (with δW2_out = 0 both runs hold the same number and decide alike) and the estimate the
reference selected has a finite bound in some channel (where it has none nothing is held to the value, so nothing needs excluding:
with w2_max = 1 a W2_out within its margin of 1 has den <= 2δden, and the pixel stays in the comparison), and (b) where the pixel
takes, or within that margin may take, the spatial estimate and one of its 7x7 taps inside the frame, of the same index and not
the centre, has dot(n(q), n) within 2·3u·Σ|n_i n'_i| of cm.  A variance-only exclusion spreads no taint: no later step reads v_out
(§4.16: "written, never read"; §4.17: the record holds m1)."""
import numpy as np

import temporal_f64
from temporal_f64 import U, VCAP
from temporal_moments_ref import MOMENTS_DEFAULTS

MISREADINGS = ("m2_from_blended_colour", "m2_blend_linear_in_c", "m2_of_squared_history", "w2_interpolated_b_squared",
               "w2_linear_weights", "w2_without_new_frame", "w2_of_history_selects", "refused_tap_in_moments", "vt_without_weight",
               "vt_without_bessel", "vt_from_interpolated", "spatial_window_5x5", "spatial_biased", "spatial_not_scaled_by_w2",
               "spatial_ignores_normals", "spatial_ignores_index", "spatial_edge_clamped_in", "min_taps_strict",
               "background_gets_the_cap", "spatial_over_accumulated_colour")
FEEDBACK_MISREADINGS = ("variance_from_fedback_colour", "write_overwrites_m1", "write_overwrites_length", "write_to_older_side",
                        "m1_from_own_record", "nonfinite_feedback_stored")
# Wrong readings of §4.23's moments step; tests/temporal_counts_f64.py lists and explains them.
COUNTS_MISREADINGS = ("neighbourhood_counts_unsampled", "centre_counted_without_samples", "m2_from_input_at_zero_count",
                      "w2_reset_at_zero_count", "w2_blended_at_zero_count")
NAMES = ("colour", "variance", "length", "W2")
# What the less obvious names switch in.  m2_from_blended_colour: m2_out = c_out².  m2_blend_linear_in_c: m2_out = fma(al, c − hq, hq),
# the colour and not its square blended into the second moment.  m2_of_squared_history: hq = h² (the interpolated colour squared instead
# of the interpolated second moment).  w2_interpolated_b_squared: HW = Σ b²·W2_q over B².  w2_linear_weights: k·hW + al.
# w2_without_new_frame: k²·hW.  w2_of_history_selects: hW > wm.  refused_tap_in_moments: Q and HW over every tap inside the frame, B over
# the accepted.  vt_without_weight: e/(1 − W2).  vt_without_bessel: e·W2.  vt_from_interpolated: e = hq − h².  spatial_biased: dp, not
# dp·S0/(S0 − 1).  spatial_edge_clamped_in: a tap outside the frame reads the nearest pixel inside.  min_taps_strict: S0 > mt.
# background_gets_the_cap: v_out = 2^32 where id < 0.  spatial_over_accumulated_colour: the centre tap adds c_out, not c.
# variance_from_fedback_colour: e from c_out on a feedback handle.  write_overwrites_length: the write stores {rgb, 0} over {c, N}.
# write_to_older_side: the write lands on the side the next step overwrites.  m1_from_own_record: h1 = m1(p), not the taps' gather.


def clamp(t):
    """§4.16's clamp(t) = !(t < 2^32) ? 2^32 : (t > 0 ? t : 0): a NaN goes to 2^32."""
    with np.errstate(invalid="ignore"):
        return np.where(~(t < VCAP), VCAP, np.where(t > 0, t, 0.0))


class TemporalMomentsF64:
    def __init__(self, width, height, feedback=False, misread=None):
        plain = misread in temporal_f64.COUNTS_MISREADINGS  # a wrong reading of §4.23's plain rules: the inner reference's
        assert misread is None or misread in MISREADINGS + COUNTS_MISREADINGS or plain or (feedback and misread in FEEDBACK_MISREADINGS), misread
        self.width, self.height, self.track, self.misread = width, height, feedback, misread
        self.inner = temporal_f64.TemporalF64(width, height, misread=misread if plain else None)
        self.state = None  # dict: m2, Em2 (h, w, 3); W2, EW (h, w); m1, Em1 (h, w, 3; a feedback handle's)
        self.last_spatial = None  # (h, w) bool: the pixels whose variance the last step took from the spatial estimate

    @property
    def last_static(self):
        return self.inner.last_static

    @property
    def last_passthrough(self):
        """The pixels whose colour, length and W2 the last step took by selection (no history: c, n, 1)."""
        return self.inner.last_passthrough

    def reset(self):
        self.inner.reset()

    def feedback(self, rgb):
        """§4.17's write: the pixels of `rgb` whose three channels are finite replace the history colour the last step wrote."""
        assert self.track, "the handle does not track feedback"
        if not self.inner.has_history:
            raise ValueError("no history to write to")
        mis = lambda name: self.misread == name  # noqa: E731
        if mis("write_to_older_side"):
            return  # (the older side is the one the next step overwrites without reading)
        img = np.asarray(rgb, np.float32).astype(np.float64).reshape(self.height, self.width, 3)
        fin = np.isfinite(img).all(axis=-1)
        if mis("nonfinite_feedback_stored"):
            fin = np.ones_like(fin)
        H, f3 = self.inner.hist, fin[..., None]
        H["c"], H["Ec"] = np.where(f3, img, H["c"]), np.where(f3, 0.0, H["Ec"])
        if mis("write_overwrites_m1"):
            self.state["m1"], self.state["Em1"] = np.where(f3, img, self.state["m1"]), np.where(f3, 0.0, self.state["Em1"])
        if mis("write_overwrites_length"):  # (a 16-byte store of {rgb, 0} into {c, N})
            H["N"], H["EN"] = np.where(fin, 0.0, H["N"]), np.where(fin, 0.0, H["EN"])

    def step(self, rgb, index, normal, point, camera, spp, bound=False, **params):
        """Returns (colour (h, w, 3), variance (h, w, 3), length (h, w), W2 (h, w)) in float64; with bound=True two more entries:
        the four bounds, shaped like the values, and (excluded, variance_excluded), each (h, w) — the second contains the first."""
        assert not (bound and self.misread), "the bound belongs to the reference as written"
        mis = lambda name: self.misread == name  # noqa: E731
        unknown = set(params) - set(temporal_f64.DEFAULTS) - set(MOMENTS_DEFAULTS)
        assert not unknown, unknown
        prm = {**MOMENTS_DEFAULTS, **params}
        wm, mt = np.float64(np.float32(prm["w2_max"])), np.float64(np.float32(prm["min_taps"]))
        plain = {k: v for k, v in params.items() if k in temporal_f64.DEFAULTS}
        cm = np.float64(np.float32({**temporal_f64.DEFAULTS, **plain}["normal_cos_min"]))
        h, w = self.height, self.width
        c = np.asarray(rgb, np.float64).reshape(h, w, 3)
        n = np.asarray(normal, np.float64).reshape(h, w, 3)
        idx = np.asarray(index).reshape(h, w).astype(np.int64)
        hit = idx >= 0

        # ---- step 1: §4.15's colour and length, from §4.15's reference ----------------------------------------------------------
        had = self.inner.has_history
        S = self.state
        counts = np.ndim(spp) != 0 and not mis("count_shared_over_the_frame")
        cnt = np.asarray(spp).reshape(h, w) if counts else None
        if self.inner.misread:  # (no bound is asked of a misreading)
            c_out, _, N_out = self.inner.step(rgb, np.zeros((h, w, 3)), index, normal, point, camera, spp, **plain)
            bc, bN, ex = np.zeros((h, w, 3)), np.zeros((h, w)), np.zeros((h, w), bool)
        else:
            c_out, _, N_out, (bc, _, bN), ex = self.inner.step(rgb, np.zeros((h, w, 3)), index, normal, point, camera, spp, bound=True, **plain)
        Ec = bc / 2
        T = self.inner.taps if had else None
        z3, z1 = np.zeros((h, w, 3)), np.zeros((h, w))

        # ---- step 2: the moments ---------------------------------------------------------------------------------------------------
        cc = c * c
        has = T["has"] if had else np.zeros((h, w), bool)
        m2_o, Em2, W2_o, EW, m1_o, Em1 = cc, U * cc, np.ones((h, w)), z1, c, z3
        hW = np.ones((h, w))
        hc = h1 = c  # (the interpolated colour history, used by one misreading)
        if had:
            with np.errstate(all="ignore"):
                g, al, da, h3 = T["gather"], T["al"], T["da0"], has[..., None]
                k = 1.0 - al
                a3, k3, da3 = al[..., None], k[..., None], da[..., None]
                how = {}
                if mis("refused_tap_in_moments"):
                    how = dict(weight=np.where(T["inside"] & T["ok"][None], T["b"], 0.0))
                hq, Ehq = g(S["m2"], S["Em2"], **how)
                if mis("w2_interpolated_b_squared"):
                    how = dict(weight=T["ba"] * T["ba"], norm=T["div"] * T["div"])
                hWb, EhW = g(S["W2"], S["EW"], **how)
                hc = T["hc"]
                if mis("m2_of_squared_history"):
                    hq = hc * hc
                if mis("m2_from_blended_colour"):
                    m2_b = c_out * c_out
                elif mis("m2_blend_linear_in_c"):
                    m2_b = a3 * (c - hq) + hq
                else:
                    m2_b = a3 * (cc - hq) + hq
                Em2_b = k3 * Ehq + np.abs(cc - hq) * da3 + a3 * (U * cc + U * np.abs(cc - hq)) + U * np.abs(m2_b)
                dk = da + U * k
                da2, dk2 = 2 * al * da + U * al * al, 2 * k * dk + U * k * k
                if mis("w2_linear_weights"):
                    W2_b = k * hWb + al
                elif mis("w2_without_new_frame"):
                    W2_b = k * k * hWb
                else:
                    W2_b = k * k * hWb + al * al
                EW_b = hWb * dk2 + k * k * EhW + da2 + U * W2_b
                if counts:
                    # §4.23: history found and n = 0 — m2_out = hq (δhq), W2_out = hW (δhW), selected on the VALUE: c may be a NaN
                    kept = cnt == 0
                    if not mis("m2_from_input_at_zero_count"):
                        m2_b, Em2_b = np.where(kept[..., None], hq, m2_b), np.where(kept[..., None], Ehq, Em2_b)
                    else:
                        m2_b, Em2_b = np.where(kept[..., None], cc, m2_b), np.where(kept[..., None], U * cc, Em2_b)
                    if mis("w2_reset_at_zero_count"):
                        W2_b = np.where(kept, 1.0, W2_b)
                    elif mis("w2_blended_at_zero_count"):
                        am = np.float64(np.float32({**temporal_f64.DEFAULTS, **plain}["alpha_min"]))
                        W2_b = np.where(kept, (1 - am) * (1 - am) * hWb + am * am, W2_b)
                    else:
                        W2_b, EW_b = np.where(kept, hWb, W2_b), np.where(kept, EhW, EW_b)
                m2_o, Em2 = np.where(h3, m2_b, m2_o), np.where(h3, Em2_b, Em2)
                W2_o, EW, hW = np.where(has, W2_b, W2_o), np.where(has, EW_b, EW), np.where(has, hWb, hW)
                if self.track:
                    if mis("m1_from_own_record"):
                        h1, Eh1 = S["m1"], S["Em1"]
                    else:
                        h1, Eh1 = g(S["m1"], S["Em1"])
                    m1_b = a3 * (c - h1) + h1
                    Em1_b = k3 * Eh1 + np.abs(c - h1) * da3 + a3 * U * np.abs(c - h1) + U * np.abs(m1_b)
                    m1_o, Em1 = np.where(h3, m1_b, m1_o), np.where(h3, Em1_b, Em1)
                    h1 = np.where(h3, h1, c)
                hc = np.where(h3, hc, c)

        # ---- step 3: the temporal estimate -----------------------------------------------------------------------------------------
        raw = self.track and not mis("variance_from_fedback_colour")
        m, Em = (m1_o, Em1) if raw else (c_out, Ec)
        with np.errstate(all="ignore"):
            h3 = has[..., None]
            if mis("vt_from_interpolated"):
                hm = h1 if raw else hc
                e = np.where(h3, hq - hm * hm, 0.0) if had else z3
            else:
                e = np.where(h3, m2_o - m * m, 0.0)  # without history: cc − cc, exactly 0 in both runs
            Ee = np.where(h3, Em2 + 2 * np.abs(m) * Em + U * m * m + U * np.abs(e), 0.0)
            ep = np.where(e > 0, e, 0.0)
            W3, EW3 = W2_o[..., None], EW[..., None]
            num = ep * W3
            Enum = W3 * Ee + ep * EW3 + U * num
            den = 1.0 - W3
            Eden = EW3 + U * den
            if mis("vt_without_weight"):
                q = ep / den
            elif mis("vt_without_bessel"):
                q = num
            else:
                q = num / den
            Evt = np.where(den - 2 * Eden > 0, (Enum + q * Eden) / (den - 2 * Eden) + U * q, np.inf)
            vt, Evt = np.where(h3, clamp(q), VCAP), np.where(h3, Evt, 0.0)

        # ---- step 4: the spatial estimate over the current frame ----------------------------------------------------------------
        vs, Evs, nnear = self._spatial(mis, c, c_out, idx, n, cm, mt, W2_o, EW, cnt)

        # ---- step 5: selection -----------------------------------------------------------------------------------------------------
        spatial = hit & ((hW if mis("w2_of_history_selects") else W2_o) > wm)
        s3 = spatial[..., None]
        v_out = np.where(hit[..., None], np.where(s3, vs, vt), VCAP if mis("background_gets_the_cap") else 0.0)
        Ev = np.where(hit[..., None], np.where(s3, Evs, Evt), 0.0)
        # (.. unless the estimate the reference selected has no finite bound in any channel: nothing is held to it then — with
        # w2_max = 1 a W2_out within its margin of 1 is exactly that case, den <= 2δden — and nothing needs excluding; the pixel
        # stays in the comparison, where only a NaN can fail)
        wnear = hit & (EW > 0) & (np.abs(W2_o - wm) <= 2 * EW) & np.isfinite(Ev).any(axis=-1)
        vex = ex | wnear | ((spatial | wnear) & nnear)

        self.state = dict(m2=m2_o, Em2=Em2, W2=W2_o, EW=EW, m1=m1_o, Em1=Em1)
        self.last_spatial = spatial
        res = (c_out, v_out, N_out, W2_o)
        if bound:
            res += ((bc, 2 * Ev, bN, 2 * EW), (ex, vex))
        return res

    def _spatial(self, mis, c, c_out, idx, n, cm, mt, W2_o, EW, cnt=None):
        """§4.16 step 4 for every pixel (the caller selects): vs, its bound, and the mask of the pixels with a 7x7 normal test inside
        its doubled margin.  With per-pixel counts `cnt` (§4.23) a position is counted only if it was sampled, the centre too."""
        h, w = self.height, self.width
        sampled = np.ones((h, w), bool) if cnt is None else cnt > 0
        sp = np.pad(sampled, 3, constant_values=True)  # (outside the frame `inside_p` decides)
        R = 2 if mis("spatial_window_5x5") else 3
        clamped = mis("spatial_edge_clamped_in")
        pad = lambda a: np.pad(a, [(3, 3), (3, 3)] + [(0, 0)] * (a.ndim - 2), mode="edge" if clamped else "constant")  # noqa: E731
        cp, npad, ip = pad(c), pad(n), pad(idx)
        inside_p = np.pad(np.ones((h, w), bool), 3, constant_values=bool(clamped))
        S0, S1, S2, A1 = np.zeros((h, w)), np.zeros((h, w, 3)), np.zeros((h, w, 3)), np.zeros((h, w, 3))
        nnear = np.zeros((h, w), bool)
        for j in range(-R, R + 1):
            for i in range(-R, R + 1):
                sl = (slice(3 + j, 3 + j + h), slice(3 + i, 3 + i + w))
                cq, nq, iq = cp[sl], npad[sl], ip[sl]
                centre = i == 0 and j == 0
                if centre and mis("spatial_over_accumulated_colour"):
                    cq = c_out
                dn = np.sum(nq * n, axis=-1)
                same = inside_p[sl] if mis("spatial_ignores_index") else inside_p[sl] & (iq == idx)
                acc = same & (centre or mis("spatial_ignores_normals") or (dn >= cm))
                if cnt is not None and not (mis("centre_counted_without_samples") if centre else mis("neighbourhood_counts_unsampled")):
                    acc = acc & sp[sl]
                    same = same & sp[sl]  # (an unsampled position's normal test decides nothing)
                if not centre:
                    nnear |= same & (np.abs(dn - cm) <= 2 * 3 * U * np.sum(np.abs(nq * n), axis=-1))
                a3 = acc[..., None]
                S0 += acc
                S1 += np.where(a3, cq, 0.0)
                S2 += np.where(a3, cq * cq, 0.0)
                A1 += np.where(a3, np.abs(cq), 0.0)
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
            if mis("spatial_biased"):
                t2, Et2 = dp, Ed
            else:
                t2 = t1 / (N0 - 1)
                Et2 = Et1 / (N0 - 1) + U * t2
            W3, EW3 = (1.0, 0.0) if mis("spatial_not_scaled_by_w2") else (W2_o[..., None], EW[..., None])
            vs = t2 * W3
            Evs = W3 * Et2 + t2 * EW3 + U * vs
            enough = (S0 > mt) if mis("min_taps_strict") else (S0 >= mt)
            e3 = enough[..., None]
            return np.where(e3, clamp(vs), VCAP), np.where(e3, Evs, 0.0), nnear


def within_bound(got, ref, hit, what, cap=0.02):
    """`temporal_f64.within_bound` for a moments step: holds its f32 outputs `got` — (colour, variance, length, W2), or (colour,
    variance) of a handle without the optional outputs — to `ref`, what `step(..., bound=True)` returned for the same inputs.  At
    most `cap` of the hit pixels in EACH mask; colour, length and W2 of every pixel outside `excluded`, and the variance of every
    pixel outside `variance_excluded`, within their bounds.  Returns the largest |difference| / bound per output (0 where both are
    0) and the two excluded shares."""
    vals, (bnds, (ex, vex)) = ref[:4], ref[4:]
    assert len(got) in (2, 4), what
    nhit = max(int(hit.sum()), 1)
    shares = float(ex[hit].sum()) / nhit, float(vex[hit].sum()) / nhit
    assert not ex[~hit].any() and not vex[~hit].any(), what
    assert shares[0] <= cap and shares[1] <= cap, f"{what}: {int(ex.sum())} (variance: {int(vex.sum())}) of {int(hit.sum())} hit pixels excluded (cap {cap})"
    ratios = []
    for name, g, x, b in zip(NAMES, got, vals, bnds):
        out = vex if name == "variance" else ex
        keep = ~out if g.ndim == 2 else np.broadcast_to(~out[..., None], g.shape)
        with np.errstate(invalid="ignore"):
            d = np.abs(np.asarray(g, np.float64) - x)
        bad = np.argwhere(keep & ~(d <= b))
        assert len(bad) == 0, f"{what} {name}: {len(bad)} values outside the bound; first at {bad[:3].tolist()}: " \
                              f"{[(float(g[tuple(i)]), float(x[tuple(i)]), float(b[tuple(i)])) for i in bad[:3]]}"
        with np.errstate(all="ignore"):
            ratios.append(float(np.where(d == 0, 0.0, d / b)[keep].max()) if keep.any() else 0.0)
    return ratios, shares
