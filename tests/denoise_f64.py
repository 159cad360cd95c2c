"""DESIGN.md §4.11 in numpy float64, written from the section's text (not from tests/denoise_mirror.cpp): vectorised over the frame
and the 25 taps, dots by `np.sum`, powers by `**`, no FMA, no fixed order of summation.  The f32 contract and this differ by
rounding only, and bound() says by how much, from this reference's own quantities.

`misread=` switches in ONE wrong reading of §4.11 (MISREADINGS); the tests require that each is told apart from the mirror.

The error bound (first order, then doubled).  u = 2^-24.  A level's output is out = Σ_q w_q e_q / W, W = Σ_q w_q.  Let the f32 run
have weights w_q + δw_q and inputs e_q + δe_q.  Since Σ_q w_q (e_q − out) = 0,

    δout = ( Σ_q (w_q + δw_q) δe_q  +  Σ_q δw_q (e_q − out) ) / (W + δW)   +  the roundings of the sums and the divide,

so to first order   |δout| <= Σ_q w_q |δe_q| / W  +  Σ_q |δw_q|·|e_q − out| / W  +  50u·Σ_q w_q |e_q| / W     (25 FMAs into S, 24 adds
into W, one divide: each at most u relative to a partial sum of like-signed terms).  |δe_q| is the previous level's bound E (the
pack's divide gives E_0 = u·|e| when it demodulates, else 0).  |δw_q| is propagated term by term from the roundings §4.11 prescribes:

    dn = dot(n_p, n_q):        |δdn| <= 3u·Σ|n_p,i n_q,i|                                  (a product and two FMAs)
    wn = max0(dn)^(2^k):       |δwn| <= 2^k (max0(dn) + |δdn|)^(2^k − 1) |δdn| + (2^k − 1) u wn   (k squarings: the relative error
                                                                                 doubles at each and gains u — why k stops at 6 here)
    v = P_q − P_p: u per component;  d2 = dot(v, v): 5u relative;  pl = dot(n_p, v):  |δpl| <= 4u·Σ|n_p,i v_i|
    r = pl² / (sp2·d2):        |δr| <= (2(|pl| + |δpl|)|δpl| + u pl²) / (sp2 d2) + 7u r
    t = max0(1 − r): |δt| <= |δr| + u;   wz = t²: |δwz| <= 2(t + |δt|)|δt| + u wz     (0 when d2 == 0;  max0 is 1-Lipschitz)
    g = wn wz:                 |δg| <= wn |δwz| + wz |δwn| + |δwn||δwz| + u g             (0 for a background pair)
    de = e_q − e_p:            |δde| <= E_q + E_p + u|de|;    de2 = dot(de, de): |δde2| <= Σ 2(|de| + |δde|)|δde| + 3u de2
    x = de2·cl / sc2:          |δx| <= cl/sc2·|δde2| + 2u x;   wc = 1 / (1 + x): |δwc| <= |δx| / (1 + x)² + 2u wc
    w = (h g) wc:              |δw| <= h (g |δwc| + wc |δg|) + 2u w

Every line is a first-order bound with the mean-value point pushed to the far end where that is free.  What is dropped is second
order — products of two of the δ above, W + δW against W — and is below the first-order terms as long as Σ|δw| << W; the final bound
is therefore DOUBLED: bound = 2·(m·E_L + u·|out|) (the last term is the rounding of ×m).  Where W itself is tiny the argument
fails, so a pixel whose W fell below 2^-20 at any level is reported in `excluded` (the tests cap their number)."""
import numpy as np

U = 2.0 ** -24
MISREADINGS = ("stride_linear", "sigma_plane_unsquared", "sigma_color_unsquared", "wz_linear", "plane_along_nq", "no_max0",
               "power_not_squaring", "colour_on_c", "colour_from_level0", "bg_weighted_zero", "normalise_by_sum_h", "kernel_box",
               "no_floor", "out_of_frame_clamped")
_K = np.array([1, 4, 6, 4, 1], np.float64) / 16
ALBEDO = 1


def denoise_f64(rgb, index, normal, point, albedo=None, *, levels=5, normal_power_log2=6, flags=ALBEDO, sigma_color=0.5,
                sigma_plane=0.25, misread=None, want_levels=None, bound=False):
    """Returns {L: out} for every L in `want_levels` (default: (levels,)), out (h, w, 3) float64 — a run of L levels is a run of
    more levels stopped early and re-modulated there.  With bound=True returns {L: (out, bound, excluded)} instead: the per-value
    error bound of the module docstring and the mask of pixels whose W was below 2^-20 at some level <= L."""
    assert misread is None or misread in MISREADINGS, misread
    assert not (bound and misread), "the bound belongs to the reference as written"
    mis = lambda name: misread == name  # noqa: E731
    want_levels = tuple(want_levels or (levels,))
    h, w = index.shape
    c = np.asarray(rgb, np.float64).reshape(h, w, 3)
    n = np.asarray(normal, np.float64).reshape(h, w, 3)
    P = np.asarray(point, np.float64).reshape(h, w, 3)
    bg = np.asarray(index).reshape(h, w) < 0
    m = np.ones((h, w, 3))
    if flags & ALBEDO:
        a = np.asarray(albedo, np.float64).reshape(h, w, 3)
        m = np.where(bg[..., None], 1.0, a if mis("no_floor") else np.maximum(a, 2.0 ** -8))
    with np.errstate(all="ignore"):
        e = c / m
        sp = np.float64(np.float32(sigma_plane))
        sc = np.float64(np.float32(sigma_color))
        sp2 = sp if mis("sigma_plane_unsquared") else np.float64(np.float32(sp) * np.float32(sp))  # host constants: f32 products
        sc2 = sc if mis("sigma_color_unsquared") else np.float64(np.float32(sc) * np.float32(sc))
        e0 = e
        E = U * np.abs(e) if (flags & ALBEDO) else np.zeros_like(e)
        excluded = np.zeros((h, w), bool)
        k1 = np.full(5, 0.2) if mis("kernel_box") else _K
        I, J = np.meshgrid(np.arange(-2, 3), np.arange(-2, 3))  # j outer, i inner (the order is immaterial here)
        I, J = I.ravel()[:, None, None], J.ravel()[:, None, None]
        hk = (k1[I + 2] * k1[J + 2])
        ys, xs = np.mgrid[0:h, 0:w]
        P2 = 2 ** normal_power_log2
        res = {}
        for l in range(max(want_levels)):
            s = 2 ** l
            cl = float(2 ** l if mis("stride_linear") else 4 ** l)
            qx, qy = xs[None] + s * I, ys[None] + s * J
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            use = np.ones_like(inside) if mis("out_of_frame_clamped") else inside
            nq, Pq, eq, bgq = n[qy, qx], P[qy, qx], e[qy, qx], bg[qy, qx]
            both, mixed = bg[None] & bgq, bg[None] ^ bgq
            dn = np.sum(n[None] * nq, axis=-1)
            dn0 = dn if mis("no_max0") else np.maximum(dn, 0.0)  # (the max0 in front of the power; the one on u stays)
            wn = dn0 ** (normal_power_log2 + 1) if mis("power_not_squaring") else dn0 ** P2
            v = Pq - P[None]
            d2 = np.sum(v * v, axis=-1)
            pl = np.sum((nq if mis("plane_along_nq") else n[None]) * v, axis=-1)
            same = d2 == 0
            r = pl * pl / np.where(same, 1.0, sp2 * d2)
            t = np.maximum(1.0 - r, 0.0)
            wz = np.where(same, 1.0, t if mis("wz_linear") else t * t)
            g = np.where(both, 1.0, wn * wz)
            if mis("colour_on_c"):
                de = eq * m[qy, qx] - (e * m)[None]
            elif mis("colour_from_level0"):
                de = e0[qy, qx] - e0[None]
            else:
                de = eq - e[None]
            de2 = np.sum(de * de, axis=-1)
            x = de2 * cl / sc2
            wc = 1.0 / (1.0 + x)
            wt = hk * g * wc
            if mis("bg_weighted_zero"):
                active = use
                wt = np.where(mixed, 0.0, wt)  # counted with weight 0: 0·e_q is added, which is NaN for a non-finite e_q
                contrib = np.where(active[..., None], wt[..., None] * eq, 0.0)
            else:
                active = use & ~mixed          # SKIPPED: neither w nor w·e_q is formed
                contrib = np.where(active[..., None], wt[..., None] * eq, 0.0)
            wt = np.where(active, wt, 0.0)
            S = np.sum(contrib, axis=0)
            W = np.sum(np.where(active, hk, 0.0), axis=0) if mis("normalise_by_sum_h") else np.sum(wt, axis=0)
            out = S / W[..., None]
            if bound:
                a3 = lambda z: np.where(active, z, 0.0)  # noqa: E731
                ddn = 3 * U * np.sum(np.abs(n[None] * nq), axis=-1)
                dwn = P2 * (dn0 + ddn) ** (P2 - 1) * ddn + (P2 - 1) * U * wn
                av = np.abs(v)
                dpl = 4 * U * np.sum(np.abs(n[None]) * av, axis=-1)
                den = np.where(same, 1.0, sp2 * d2)
                dr = (2 * (np.abs(pl) + dpl) * dpl + U * pl * pl) / den + 7 * U * r
                dt = dr + U
                dwz = np.where(same, 0.0, 2 * (t + dt) * dt + U * wz)
                dg = np.where(both, 0.0, wn * dwz + wz * dwn + dwn * dwz + U * g)
                dde = E[qy, qx] + E[None] + U * np.abs(de)
                dde2 = np.sum(2 * (np.abs(de) + dde) * dde, axis=-1) + 3 * U * de2
                dx = cl / sc2 * dde2 + 2 * U * x
                dwc = dx / (1 + x) ** 2 + 2 * U * wc
                dw = a3(hk * (g * dwc + wc * dg) + 2 * U * wt)
                sel = lambda z: np.where(active[..., None], z, 0.0)  # noqa: E731
                E = (np.sum(sel(wt[..., None] * E[qy, qx]), axis=0) + np.sum(sel(dw[..., None] * np.abs(eq - out[None])), axis=0)
                     + 50 * U * np.sum(sel(wt[..., None] * np.abs(eq)), axis=0)) / W[..., None]
                excluded = excluded | ~(W >= 2.0 ** -20)
            e = out
            if l + 1 in want_levels:
                fin = e * m
                res[l + 1] = (fin, 2 * (m * E + U * np.abs(fin)), excluded.copy()) if bound else fin
    return res
