"""DESIGN.md §4.13 in numpy float64, written from the section's text and from the parts of §4.11 it inherits (not from
tests/denoise_guided_mirror.cpp, not from the kernels): vectorised over the frame, the 9 prefilter taps and the 25 taps, sums by
`np.sum`, powers by `**`, no FMA, no fixed order of summation.  The host constants `sp2`, `sc2` and `vf` are the f32 values the
contract prescribes, widened.  The f32 contract and this differ by rounding only, and the bounds say by how much, from this
reference's own quantities.  The geometry term `g` and its error are §4.11's, restated here as tests/denoise_f64.py states them.

`misread=` switches in ONE wrong reading of §4.13 (MISREADINGS); the tests require that each is told apart from the mirror.

The error bound (first order, then doubled).  u = 2^-24; η = 2^-149 stands for the absolute error of an f32 result that lands below
2^-126 (where the error is no longer u relative): it is added where a product of weights can get that small — `w`, `w·w`, the sums
into `V`, `de2` — and is invisible everywhere else.  E is the bound on a level's input colour (per channel), D the bound on its
input variance; both are absolute and per pixel, because variances of one frame span 0 .. 2^32.

  Pack (§4.13 "Pack").  e = c / m: E_0 = u·|e| when the run demodulates, else 0 (§4.11).  q_ch = var_ch / (m_ch·m_ch) is a product
  and a divide, 2u relative; t = (q_r + q_g) + q_b is two adds, each u relative to a partial sum that is at most Σ|q_ch| (a negative
  variance makes the terms of mixed sign, hence the absolute values): |δt| <= 4u·Σ|q_ch|.  v = clamp(t) and the clamp is 1-Lipschitz:
  |δv| <= |δt|, D_0 = |δt|; D_0 = 0 where t is not finite (both sides give VCAP exactly), where t − |δt| >= VCAP (both give VCAP) and
  where t + |δt| <= 0 (both give 0).

  Prefilter (§4.13 "First the variance is prefiltered").  G is a sum of at most nine dyadics: exact.  A = Σ gg·v_q by nine FMAs, each
  u relative to a partial sum of non-negative terms, from inputs v_q + δv_q:  |δA| <= Σ gg·D_q + 9u·A.  gv = A / G:
      |δgv| <= Σ gg·D_q / G + 10u·gv.
  den = sc2·(gv + vf), an add and a product:  |δden| / den <= |δgv| / (gv + vf) + 2u =: ρ   (sc2 = +inf: den = +inf on both sides).

  Colour weight (§4.13 "de = e_q − e_p ...").  de and de2 as in §4.11: |δde| <= E_q + E_p + u|de|, |δde2| <= Σ 2(|de| + |δde|)|δde| +
  3u·de2 + 4η.  x = de2 / den: |δx| <= |δde2| / den + x·(ρ + u) + η   (0 when sc2 = +inf: x = 0 exactly).  wc = 1 / (1 + x):
  |δwc| <= |δx| / (1 + x)² + 2u·wc — except at the CENTRE tap, where the f32 run subtracts e_p from itself: de = 0, x = 0 and wc = 1
  with no error at all ("the centre tap contributes 9/64·g_c with wc = 1"), whatever E_p is; that matters where den is tiny (a
  converged pixel over a small var_floor), because E_p² / den is then not small and the centre tap carries most of W.
  w = (h·g)·wc: |δw| <= h·(g·|δwc| + wc·|δg|) + 2u·w + η, with |δg| from §4.11's lines for dn, wn, v, d2, pl, r, t, wz and g, unchanged.

  Colour (§4.13 "The level's output colour is S_ch / W").  §4.11's argument word for word, since Σ_q w_q (e_q − out) = 0:
      E' = ( Σ_q w_q E_q + Σ_q |δw_q|·|e_q − out| + 50u·Σ_q w_q |e_q| ) / W.

  Variance (§4.13 "V = fma(w·w, v_q, V)", "V / (W·W)").  out_v = Σ_q w_q² v_q / (Σ_q w_q)², so ∂out_v / ∂w_q = 2 (w_q v_q − out_v·W) / W²:
  the error of w enters TWICE, through V and through W·W, and the two partly cancel, which this form keeps.  The input error enters
  weighted by w²; the roundings are: w·w (u), 25 FMAs into V (each u relative to a partial sum of non-negative terms: 25u·V), 24 adds
  into W (24u, entering squared: 48u), the product W·W (u) and the divide (u): 76u·out_v in all.  Hence
      D' = ( Σ_q w_q² D_q + 2 Σ_q |δw_q|·|w_q v_q − out_v·W| ) / W²  +  76u·out_v  +  η·(Σ_q v_q + 25) / W² + η.

Every line is a first-order bound with the mean-value point pushed to the far end where that is free.  What is dropped is second
order — products of two of the δ above, W + δW against W, den + δden against den — and is below the first-order terms as long as
Σ|δw| << W and |δden| << den; the final bounds are therefore DOUBLED: colour 2·(m·E_L + u·|out|) (the last term is the rounding of
×m), variance 2·D_L (the variance output is the level's own divide, stored as it is).

Where the first-order argument fails a pixel is reported in `excluded` (the tests cap their number):
  * W < 2^-20 at some level, as in §4.11: with unit normals §4.13 promises W >= 9/64, so this marks a degenerate guide;
  * |δgv| > 2^-6·(gv + vf) at some level: x = de2 / den is expanded in ρ = δden / den, and the term dropped is ρ times the one
    kept; at 2^-6 the doubling is still nearly whole for everything else.  ρ is small where δgv, an average of the neighbours' D,
    stands against an average of their variances plus vf and D is a few hundred u of its variance.  It grows where a pixel's
    variance arrives mostly through a tap of tiny, ill-conditioned weight (wz = t·t near t = 0 has the relative error 2u / t) from
    a neighbour at VCAP: D is then honest but no longer tiny against the variance, later levels hand it on through ρ, and with a
    small `var_floor` nothing else holds `den` up (largest ρ met on the tests' synthetic frames: 2.0·10^-3, var_floor 1e-8).
The bound is for inputs on which f32 `den` stays finite (asserted: den < 2^126, or den = +inf through sc2 = +inf, where both sides
have x = 0 exactly); what a `den` that OVERFLOWS does is pinned exactly by the hand case `step-vcap` of
tests/denoise_guided_cases.py, not here.

A misreading considered and left out because it is another one by construction: "G counts the skipped taps too" makes G the sum of
all nine gg, which is 1, so gv = A — `prefilter_unnormalised` to the last bit."""
import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -149
VCAP = 2.0 ** 32
ALBEDO = 1
MISREADINGS = ("prefilter_at_stride", "prefilter_off", "prefilter_across_background", "prefilter_unnormalised", "prefilter_box",
               "prefilter_from_packed", "den_of_tap", "keeps_4l", "floor_outside", "sigma_color_unsquared", "colour_on_c",
               "weights_not_squared", "variance_over_W", "variance_from_packed", "variance_not_demodulated", "variance_demodulated_by_m",
               "variance_mean_of_channels", "nan_to_zero", "negative_by_magnitude", "var_out_remodulated",
               # two more that reading §4.13 suggests: a finite t >= VCAP kept as it is; an out-of-frame prefilter tap clamped to the border
               "vcap_passes_huge", "prefilter_clamped_at_border")
_K = np.array([1, 4, 6, 4, 1], np.float64) / 16
_GK = np.array([1, 2, 1], np.float64) / 4


def pack_f64(rgb, var_rgb, index, albedo=None, *, flags=ALBEDO, misread=None):
    """§4.13's pack pass: (m (h, w, 3), e (h, w, 3), v (h, w), D_0 (h, w)) — the modulation, the demodulated colour, the clamped
    variance and the bound on its f32 value."""
    mis = lambda name: misread == name  # noqa: E731
    h, w = index.shape
    c = np.asarray(rgb, np.float64).reshape(h, w, 3)
    var = np.asarray(var_rgb, np.float64).reshape(h, w, 3)
    bg = np.asarray(index).reshape(h, w) < 0
    m = np.ones((h, w, 3))
    if flags & ALBEDO:
        m = np.where(bg[..., None], 1.0, np.maximum(np.asarray(albedo, np.float64).reshape(h, w, 3), 2.0 ** -8))
    with np.errstate(all="ignore"):
        e = c / m
        q = var if mis("variance_not_demodulated") else var / m if mis("variance_demodulated_by_m") else var / (m * m)
        t = (q[..., 0] + q[..., 1]) + q[..., 2]
        if mis("variance_mean_of_channels"):
            t = t / 3
        if mis("negative_by_magnitude"):
            t = np.abs(t)
        capped = ~np.isfinite(t) & ~(t == -np.inf) if mis("vcap_passes_huge") else ~(t < VCAP)
        v = np.where(capped, VCAP, np.where(t > 0, t, 0.0))
        if mis("nan_to_zero"):
            v = np.where(np.isnan(t) | (t == np.inf), 0.0, v)
        dt = 4 * U * np.sum(np.abs(q), axis=-1)
        D = np.where(np.isfinite(t) & np.isfinite(dt), dt, 0.0)
        D = np.where((t - D >= VCAP) | (t + D <= 0), 0.0, D)
    return m, e, v, D


def denoise_guided_f64(rgb, var_rgb, index, normal, point, albedo=None, *, levels=5, normal_power_log2=6, flags=ALBEDO, sigma_color=2.0,
                       sigma_plane=0.25, var_floor=1e-4, want_levels=None, misread=None, bound=False):
    """Returns {L: (colour (h, w, 3), variance (h, w))} for every L in `want_levels` (default: (levels,)), float64 — a run of L levels
    is a run of more levels stopped early, its colour re-modulated there.  With bound=True returns {L: (colour, colour_bound,
    variance, variance_bound, excluded)}: the per-value bounds of the module docstring and the mask of pixels where its first-order
    argument failed at some level <= L."""
    assert misread is None or misread in MISREADINGS, misread
    assert not (bound and misread), "the bound belongs to the reference as written"
    mis = lambda name: misread == name  # noqa: E731
    want_levels = tuple(want_levels or (levels,))
    h, w = index.shape
    n = np.asarray(normal, np.float64).reshape(h, w, 3)
    P = np.asarray(point, np.float64).reshape(h, w, 3)
    bg = np.asarray(index).reshape(h, w) < 0
    m, e, v, D = pack_f64(rgb, var_rgb, index, albedo, flags=flags, misread=misread)
    v0 = v
    with np.errstate(all="ignore"):
        sp = np.float32(sigma_plane)
        sc = np.float32(sigma_color)
        sp2 = np.float64(sp * sp)  # host constants: f32 products
        sc2 = np.float64(sc) if mis("sigma_color_unsquared") else np.float64(sc * sc)
        vf = np.float64(np.float32(var_floor))
        E = U * np.abs(e) if (flags & ALBEDO) else np.zeros_like(e)
        excluded = np.zeros((h, w), bool)
        I, J = np.meshgrid(np.arange(-2, 3), np.arange(-2, 3))  # j outer, i inner (the order is immaterial here)
        I, J = I.ravel()[:, None, None], J.ravel()[:, None, None]
        hk = _K[I + 2] * _K[J + 2]
        centre = (I == 0) & (J == 0)
        GI, GJ = np.meshgrid(np.arange(-1, 2), np.arange(-1, 2))
        GI, GJ = GI.ravel()[:, None, None], GJ.ravel()[:, None, None]
        gg = np.full((9, 1, 1), 1.0 / 9) if mis("prefilter_box") else _GK[GI + 1] * _GK[GJ + 1]
        ys, xs = np.mgrid[0:h, 0:w]
        P2 = 2 ** normal_power_log2
        res = {}
        for l in range(max(want_levels)):
            s = 2 ** l
            # ---- the prefilter: 3x3 at distance 1, taps outside the frame or across the background border skipped, A / G
            ps = s if mis("prefilter_at_stride") else 1
            px, py = xs[None] + ps * GI, ys[None] + ps * GJ
            pin = (px >= 0) & (px < w) & (py >= 0) & (py < h)
            px, py = np.clip(px, 0, w - 1), np.clip(py, 0, h - 1)
            ok = np.ones_like(pin) if mis("prefilter_clamped_at_border") else pin
            if not mis("prefilter_across_background"):
                ok = ok & (bg[py, px] == bg[None])
            pv = (v0 if mis("prefilter_from_packed") else v)[py, px]
            G = np.sum(np.where(ok, gg, 0.0), axis=0)
            A = np.sum(np.where(ok, gg * pv, 0.0), axis=0)
            gv = v if mis("prefilter_off") else A if mis("prefilter_unnormalised") else A / G
            # ---- the 25 taps
            qx, qy = xs[None] + s * I, ys[None] + s * J
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            nq, Pq, eq, bgq = n[qy, qx], P[qy, qx], e[qy, qx], bg[qy, qx]
            both, mixed = bg[None] & bgq, bg[None] ^ bgq
            active = inside & ~mixed           # a background-versus-hit tap is SKIPPED: neither w nor w·e_q is formed
            dn = np.sum(n[None] * nq, axis=-1)
            dn0 = np.maximum(dn, 0.0)
            wn = dn0 ** P2
            d = Pq - P[None]
            d2 = np.sum(d * d, axis=-1)
            pl = np.sum(n[None] * d, axis=-1)
            same = d2 == 0
            r = pl * pl / np.where(same, 1.0, sp2 * d2)
            t = np.maximum(1.0 - r, 0.0)
            wz = np.where(same, 1.0, t * t)
            g = np.where(both, 1.0, wn * wz)
            de = eq * m[qy, qx] - (e * m)[None] if mis("colour_on_c") else eq - e[None]
            de2 = np.sum(de * de, axis=-1)
            gvt = gv[qy, qx] if mis("den_of_tap") else gv[None]
            den = sc2 * gvt + vf if mis("floor_outside") else sc2 * (gvt + vf)
            x = (de2 * 4.0 ** l if mis("keeps_4l") else de2) / den
            wc = 1.0 / (1.0 + x)
            wt = np.where(active, hk * g * wc, 0.0)
            vq = (v0 if mis("variance_from_packed") else v)[qy, qx]
            W = np.sum(wt, axis=0)
            S = np.sum(np.where(active[..., None], wt[..., None] * eq, 0.0), axis=0)
            out = S / W[..., None]
            if mis("weights_not_squared"):
                vout = np.sum(np.where(active, wt * vq, 0.0), axis=0) / W
            else:
                V = np.sum(np.where(active, wt * wt * vq, 0.0), axis=0)
                vout = V / W if mis("variance_over_W") else V / (W * W)
            if bound:
                assert np.isinf(sc2) or (den < 2.0 ** 126).all(), "f32 den would overflow: outside the bound's range"
                a3 = lambda z: np.where(active, z, 0.0)  # noqa: E731
                sel = lambda z: np.where(active[..., None], z, 0.0)  # noqa: E731
                dgv = np.sum(np.where(ok, gg * D[py, px], 0.0), axis=0) / G + 10 * U * gv
                rho = dgv / (gv + vf) + 2 * U
                ddn = 3 * U * np.sum(np.abs(n[None] * nq), axis=-1)
                dwn = P2 * (dn0 + ddn) ** (P2 - 1) * ddn + (P2 - 1) * U * wn
                dpl = 4 * U * np.sum(np.abs(n[None]) * np.abs(d), axis=-1)
                dr = (2 * (np.abs(pl) + dpl) * dpl + U * pl * pl) / np.where(same, 1.0, sp2 * d2) + 7 * U * r
                dt = dr + U
                dwz = np.where(same, 0.0, 2 * (t + dt) * dt + U * wz)
                dg = np.where(both, 0.0, wn * dwz + wz * dwn + dwn * dwz + U * g)
                dde = E[qy, qx] + E[None] + U * np.abs(de)
                dde2 = np.sum(2 * (np.abs(de) + dde) * dde, axis=-1) + 3 * U * de2 + 4 * ETA
                dx = np.zeros_like(x) if np.isinf(sc2) else dde2 / den + x * (rho[None] + U) + ETA
                dwc = np.where(centre, 0.0, dx / (1 + x) ** 2 + 2 * U * wc)  # the centre tap: e_p − e_p = 0 and 1 / (1 + 0) = 1, exactly
                dw = a3(hk * (g * dwc + wc * dg) + 2 * U * wt + ETA)
                E = (np.sum(sel(wt[..., None] * E[qy, qx]), axis=0) + np.sum(sel(dw[..., None] * np.abs(eq - out[None])), axis=0)
                     + 50 * U * np.sum(sel(wt[..., None] * np.abs(eq)), axis=0)) / W[..., None]
                WW = W * W
                D = ((np.sum(a3(wt * wt * D[qy, qx]), axis=0) + 2 * np.sum(dw * np.abs(a3(wt * vq) - (vout * W)[None]), axis=0)) / WW
                     + 76 * U * vout + ETA * (np.sum(a3(vq), axis=0) + 25) / WW + ETA)
                excluded = excluded | ~(W >= 2.0 ** -20)
                if not np.isinf(sc2):
                    excluded = excluded | ~(dgv <= 2.0 ** -6 * (gv + vf))
            e, v = out, vout
            if l + 1 in want_levels:
                fin = e * m
                vfin = v * m[..., 0] if mis("var_out_remodulated") else v
                res[l + 1] = (fin, 2 * (m * E + U * np.abs(fin)), vfin, 2 * D, excluded.copy()) if bound else (fin, vfin)
    return res
