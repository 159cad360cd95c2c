"""DESIGN.md §4.20 in numpy float64 — the run on block means and the run with a phase ("Lattice samples") —, written from the
section's text and from the parts of §4.11 and §4.13 it inherits (not from tests/upscale_mirror.cpp, tests/upscale_phase_mirror.cpp
or the kernels): vectorised over the frame and the taps, sums by `np.sum`, powers by `**`, no FMA, no fixed order of summation.

Two things are stated differently from the section, so that this is a second reading and not a copy.
  POSITION comes from geometry, not from §4.20's integer formulas.  In low-resolution pixel coordinates full pixel x lies at
  (x + 1/2)/f − 1/2 in the run on block means (low-resolution pixel i looks at the centre of its block of f full pixels) and at
  (x − px)/f in the run with a phase (low-resolution pixel i IS full pixel f·i + px); i0 is the floor of that and fx its fractional
  part.  Both are exact in float64 wherever the result is an integer or a dyadic (always at f = 2 and 4; on the samples at f = 3), so `b == 0`
  and "sampled" are decided as the integers decide them.  The nearest sample of stage 2 is the argmin of |x − sample position|, a
  tie going to the right (there is none on block means).
  THE GUIDE WEIGHT g is §4.11's, restated with the upscaler's roles: p, the centre, whose normal and point define the tangent
  plane `pl` is measured from, is the FULL pixel; q, the tap, is the low-resolution one.
`sp2` is the f32 product the contract prescribes, widened.

`misread=` switches in ONE wrong reading of §4.20 (MISREADINGS); the tests require that each is told apart from the mirrors.

The error bound (first order, then doubled).  u = 2^-24; η = 2^-149 stands for the absolute error of an f32 result that lands below
2^-126: it is added where a product of weights can get that small (cos^64, w = b·g, w·w, the sums into acc and V, W·W).

  Pack.  e = c / m: E_q = u·|e_q| when the run demodulates, else 0.  t = var / (m·m) per channel is a product and a divide: 2u·|t| + η,
  and 0 where m = 1 (both operations exact).  ve = clamp_var(t), 1-Lipschitz: D_q = |δt|; D_q = 0 where t is not finite (both sides
  give 2^32), where t − |δt| >= 2^32 and where t + |δt| <= 0 (both give 0).
  Position.  The one rounding the contract puts on fx is f32(r) / f32(2f) resp. f32(r) / f32(f): exact for f = 2 and 4, at most
  u·fx for f = 3.  1 − fx is then exact for f = 2 and 4 and rounds once more for f = 3: |δ(1 − fx)| <= u·fx + u·(1 − fx) = u.  So with
  τ = [f = 3]: |δbx| <= τ·u·fx (di = 1), τ·u (di = 0).  b = bx·by, one product: |δb| <= by·|δbx| + bx·|δby| + u·b.  In stage 1 b = 1 exactly.
  Guide weight.  §4.11's lines as tests/denoise_f64.py states them, p the full pixel:
      dn = dot(n_p, n_q):    |δdn| <= 3u·Σ|n_p,i n_q,i|
      wn = max0(dn)^(2^k):   |δwn| <= 2^k (max0(dn) + |δdn|)^(2^k − 1) |δdn| + (2^k − 1) u wn
      v = P_q − P_p: u per component;  d2 = dot(v, v): 5u relative;  pl = dot(n_p, v): |δpl| <= 4u·Σ|n_p,i v_i|
      r = pl² / (sp2·d2):    |δr| <= (2(|pl| + |δpl|)|δpl| + u pl²) / (sp2 d2) + 7u r
      t = max0(1 − r): |δt| <= |δr| + u;   wz = t²: |δwz| <= 2(t + |δt|)|δt| + u wz   (0 when d2 == 0)
      g = wn wz:             |δg| <= wn |δwz| + wz |δwn| + |δwn||δwz| + u g + η       (0 for a background pair)
  max0 is 1-Lipschitz, and where its argument is negative by more than twice its own error both sides give 0 exactly: |δwn| = 0 where
  dn + 2|δdn| <= 0, |δt| = 0 where 1 − r + 2(|δr| + u) <= 0 (another surface far off the tangent plane: r is in the thousands).  η is
  added only where the product can be non-zero on either side (wn + |δwn| > 0 and wz + |δwz| > 0): 0·x = 0 exactly.
  Weight.  w = b·g: |δw| <= b|δg| + g|δb| + u·w + η (η again only where g + |δg| > 0).
  Colour.  Σ_q w_q (e_q − ē) = 0 with ē = acc / W, so with T = 4 (stage 0) or 16 (stage 1) taps — T FMAs into acc, T adds into W,
  one divide, each at most u relative to a partial sum of like-signed terms —
      |δē| <= ( Σ_q w_q E_q + Σ_q |δw_q|·|e_q − ē| + (T + 1)u·Σ_q w_q |e_q| + T·η ) / W,
  and out = ē·m_p is one more rounding (m_p is a selection of an input, or a max with a constant: exact): colour bound
  2·(m_p·|δē| + u·|out|).
  Variance.  §4.13's form: v̄ = Σ w_q² ve_q / (Σ w_q)² has ∂v̄/∂w_q = 2 (w_q ve_q − v̄·W) / W²; the error of w enters through V and
  through W·W and the two partly cancel, which this keeps.  Roundings: w·w (u), T FMAs into V (T·u), T − 1 adds into W entering
  twice (2(T − 1)u), W·W (u), the divide (u), m_p·m_p (u), the last product (u): (3T + 3)u in all, 15u and 51u.  η: on every w·w
  (times ve_q), on every FMA into V, on W·W (relative η / W², i.e. v̄·η / W² absolute).  Hence, in demodulated units,
      |δv̄| <= ( Σ_q w_q² D_q + 2 Σ_q |δw_q|·|w_q ve_q − v̄·W| + η·(Σ_q ve_q + T + v̄) ) / W²  + η,
  variance bound 2·(m_p²·|δv̄| + (3T + 3)u·var).
  By selection.  Stage 2 (the nearest pixel's raw colour, variance 2^32) and a sampled pixel passed through in the run with a phase
  (raw colour, clamp_var of the raw variance) are selections: their bound is 0 and the comparison there is for equality.

What is dropped is second order and is below the first-order terms as long as Σ|δw| << W; hence the doubling.  `excluded` marks the
pixels where a DECISION lies within the doubled propagated error of its border, or where the first-order argument fails:
  * W >= 2^-40 after stage 0, and after stage 1 for the pixels that get there: |W − 2^-40| <= 2·Σ|δw|.  (A pixel with no tap on
    its own surface leaves a stage with W = 0 and Σ|δw| = 0, or far below 2^-40: no doubt there.)
  * in the run with a phase, a sampled pixel's g > 0: g <= 2|δg| (unless both are 0);
  * Σ|δw| > 2^-6·W in the stage that produced the pixel (the sibling modules' first-order threshold).
Everything else is exact on both sides (b == 0, d2 == 0 on identical f32 inputs, inside or outside the frame, bg) or Lipschitz and
bounded (max0, clamp_var).  At every pixel that is not excluded the stage map must be EQUAL.

Misreadings considered and left out:
  * `distance_from_tap_plane_and_point_swapped` (the distance of P_p from q's tangent plane, dot(n_q, P_p − P_q)) is
    `plane_along_nq` by construction: pl changes its sign and only pl·pl is used.
  * A sampled pixel REBUILT through the divide instead of passed through — ((g·(c/m_q)) / g)·m_p — differs by three roundings and
    lies inside any honest bound; the hand case `sampled_raw_f2_p01` of tests/upscale_phase_cases.py holds it exactly, bit for bit."""
import numpy as np

U = 2.0 ** -24
ETA = 2.0 ** -149
VCAP = 2.0 ** 32
WMIN = 2.0 ** -40  # a stage is taken with W >= 2^-40
ALBEDO = 1
MISREADINGS = (
    # position, the run on block means
    "lowres_pixel_at_corner", "footprint_from_x_div_f",
    # centre and tap
    "plane_along_nq", "centre_guides_from_lowres",
    # modulation
    "modulate_with_lowres_albedo", "taps_not_demodulated", "no_floor", "background_demodulated",
    # weights inherited from §4.11
    "wz_linear", "power_not_squaring", "sigma_plane_unsquared", "no_max0",
    # taps
    "out_of_frame_clamped", "both_background_skipped",
    # stages
    "stage1_keeps_bilinear", "stage1_3x3_about_nearest", "stage2_modulated", "stage2_variance_from_input", "stage1_never",
    # variance
    "weights_not_squared", "variance_over_W", "variance_modulated_by_m", "variance_demodulated_by_m", "variance_not_clamped",
    # the run with a phase
    "phase_uses_block_position", "phase_ignored", "nearest_is_x_div_f", "tie_to_the_left", "sample_passes_when_refused")


def _clamp_var(t):
    return np.where(~(t < VCAP), VCAP, np.where(t > 0, t, 0.0))


def _axis(n_full, n_lo, f, p, mis):
    """One axis: (i0, fx, nearest sample) per full pixel, from where the full pixels and the samples lie."""
    x = np.arange(n_full, dtype=np.float64)
    block = (x + 0.5) / f - 0.5
    if p is None:
        pos = x / f if mis("lowres_pixel_at_corner") else block
        samples = (np.arange(n_lo) + 0.5) * f - 0.5  # the block centres, in full-pixel coordinates
    else:
        pos = block if mis("phase_uses_block_position") else (x - p) / f
        samples = f * np.arange(n_lo, dtype=np.float64) + p
    i0 = np.floor(pos)
    fx = pos - i0
    if p is None and mis("footprint_from_x_div_f"):
        i0 = np.floor(x / f)
    d = np.abs(x[:, None] - samples[None, :])
    near = np.argmin(d, axis=1) if mis("tie_to_the_left") else n_lo - 1 - np.argmin(d[:, ::-1], axis=1)
    if p is not None and mis("nearest_is_x_div_f"):
        near = np.arange(n_full) // f
    return i0.astype(np.int64), fx, near.astype(np.int64)


def upscale_f64(rgb_lo, g_lo, g_hi, factor, var_rgb=None, phase=None, *, normal_power_log2=6, flags=ALBEDO, sigma_plane=0.25,
                misread=None, bound=False, detail=None):
    """`g_lo`, `g_hi`: anything with .index (h, w), .normal, .point and (with ALBEDO) .albedo (h, w, 3).  Returns (out (H, W, 3),
    var (H, W, 3) or None, stage (H, W)) in float64 / uint8; with bound=True (out, out_bound, var, var_bound, stage, excluded): the
    per-value bounds of the module docstring (0 where the value is a selection) and the mask of pixels where a decision is in doubt
    or the first-order argument fails.  `detail`: a dict that receives the stage-0 taps' guide weights `g0` and the mask `accepted0`
    of the taps that were not skipped, both (4, H, W) — what the tests state their conditions on the inputs with."""
    assert misread is None or misread in MISREADINGS, misread
    assert not (bound and misread), "the bound belongs to the reference as written"
    mis = lambda name: misread == name  # noqa: E731
    f = int(factor)
    if phase is not None and mis("phase_ignored"):
        phase = (0, 0)
    h, w = np.asarray(g_lo.index).shape
    H, W_ = np.asarray(g_hi.index).shape
    assert (H, W_) == (f * h, f * w)
    demod = bool(flags & ALBEDO)
    c = np.asarray(rgb_lo, np.float64).reshape(h, w, 3)
    have_var = var_rgb is not None
    n_lo, P_lo, bg_lo = np.asarray(g_lo.normal, np.float64), np.asarray(g_lo.point, np.float64), np.asarray(g_lo.index) < 0
    n_hi, P_hi, bg_hi = np.asarray(g_hi.normal, np.float64), np.asarray(g_hi.point, np.float64), np.asarray(g_hi.index) < 0

    def modulation(g, bg):
        if not demod:
            return np.ones(bg.shape + (3,))
        a = np.asarray(g.albedo, np.float64)
        m = a if mis("no_floor") else np.maximum(a, 2.0 ** -8)
        return m if mis("background_demodulated") else np.where(bg[..., None], 1.0, m)

    with np.errstate(all="ignore"):
        sp = np.float32(sigma_plane)
        sp2 = np.float64(sp) if mis("sigma_plane_unsquared") else np.float64(sp * sp)  # the host constant: an f32 product
        # ---- pack
        m_lo, m_hi = modulation(g_lo, bg_lo), modulation(g_hi, bg_hi)
        e = c if mis("taps_not_demodulated") else c / m_lo
        E = U * np.abs(e) if demod else np.zeros_like(e)
        ve = D = None
        if have_var:
            var_in = np.asarray(var_rgb, np.float64).reshape(h, w, 3)
            t = var_in / m_lo if mis("variance_demodulated_by_m") else var_in / (m_lo * m_lo)
            ve = t if mis("variance_not_clamped") else _clamp_var(t)
            dt = np.where(m_lo == 1.0, 0.0, 2 * U * np.abs(t) + ETA)
            D = np.where(np.isfinite(t) & np.isfinite(dt), dt, 0.0)
            D = np.where((t - D >= VCAP) | (t + D <= 0), 0.0, D)
        # ---- position
        i0, fx, near_x = _axis(W_, w, f, None if phase is None else phase[0], mis)
        j0, fy, near_y = _axis(H, h, f, None if phase is None else phase[1], mis)
        I0, J0 = np.broadcast_to(i0[None, :], (H, W_)), np.broadcast_to(j0[:, None], (H, W_))
        FX, FY = np.broadcast_to(fx[None, :], (H, W_)), np.broadcast_to(fy[:, None], (H, W_))
        NX, NY = np.broadcast_to(near_x[None, :], (H, W_)), np.broadcast_to(near_y[:, None], (H, W_))
        tau = 1.0 if f == 3 else 0.0
        # ---- the centre: the full pixel
        if mis("centre_guides_from_lowres"):
            ys, xs = np.mgrid[0:H, 0:W_]
            n_p, P_p = n_lo[ys // f, xs // f], P_lo[ys // f, xs // f]
        else:
            n_p, P_p = n_hi, P_hi
        m_p = m_lo[NY, NX] if mis("modulate_with_lowres_albedo") else m_hi
        P2 = 2 ** normal_power_log2

        def taps(I, J, b, db, T):
            """The sums over the taps (I, J) (T, H, W) with the position weights b: a dict of the section's quantities, and with
            `bound` their propagated errors."""
            inside = (I >= 0) & (I < w) & (J >= 0) & (J < h)
            qi, qj = np.clip(I, 0, w - 1), np.clip(J, 0, h - 1)
            use = np.ones_like(inside) if mis("out_of_frame_clamped") else inside
            nq, Pq, bgq, eq = n_lo[qj, qi], P_lo[qj, qi], bg_lo[qj, qi], e[qj, qi]
            both, mixed = bg_hi[None] & bgq, bg_hi[None] ^ bgq
            dn = np.sum(n_p[None] * nq, axis=-1)
            dn0 = dn if mis("no_max0") else np.maximum(dn, 0.0)  # (the max0 in front of the power; the one on 1 − r stays)
            wn = dn0 ** (normal_power_log2 + 1) if mis("power_not_squaring") else dn0 ** P2
            v = Pq - P_p[None]
            d2 = np.sum(v * v, axis=-1)
            pl = np.sum((nq if mis("plane_along_nq") else n_p[None]) * v, axis=-1)
            same = d2 == 0
            den = np.where(same, 1.0, sp2 * d2)
            r = pl * pl / den
            t = np.maximum(1.0 - r, 0.0)
            wz = np.where(same, 1.0, t if mis("wz_linear") else t * t)
            g = np.where(both, 1.0, wn * wz)
            active = use & (b != 0) & ~mixed  # a background-versus-hit tap is SKIPPED
            if mis("both_background_skipped"):
                active = active & ~both
            wt = np.where(active, b * g, 0.0)
            a3 = lambda z: np.where(active, z, 0.0)  # noqa: E731
            sel = lambda z: np.where(active[..., None], z, 0.0)  # noqa: E731
            Wsum = np.sum(wt, axis=0)
            acc = np.sum(sel(wt[..., None] * eq), axis=0)
            ebar = acc / Wsum[..., None]
            res = dict(W=Wsum, ebar=ebar, g=g, active=active, wt=wt)
            if have_var:
                vq = ve[qj, qi]
                if mis("weights_not_squared"):
                    vbar = np.sum(sel(wt[..., None] * vq), axis=0) / Wsum[..., None]
                else:
                    V = np.sum(sel((wt * wt)[..., None] * vq), axis=0)
                    vbar = V / Wsum[..., None] if mis("variance_over_W") else V / (Wsum * Wsum)[..., None]
                res["vbar"] = vbar
            if bound:
                ddn = 3 * U * np.sum(np.abs(n_p[None] * nq), axis=-1)
                ddn = np.where(dn + 2 * ddn <= 0, 0.0, ddn)
                dwn = P2 * (dn0 + ddn) ** (P2 - 1) * ddn + (P2 - 1) * U * wn
                dpl = 4 * U * np.sum(np.abs(n_p[None]) * np.abs(v), axis=-1)
                dr = (2 * (np.abs(pl) + dpl) * dpl + U * pl * pl) / den + 7 * U * r
                dt_ = dr + U
                dt_ = np.where(1.0 - r + 2 * dt_ <= 0, 0.0, dt_)
                dwz = np.where(same, 0.0, 2 * (t + dt_) * dt_ + U * wz)
                alive = (wn + dwn > 0) & (wz + dwz > 0)
                dg = np.where(both, 0.0, wn * dwz + wz * dwn + dwn * dwz + U * g + np.where(alive, ETA, 0.0))
                dw = a3(b * dg + g * db + U * wt + np.where(g + dg > 0, ETA, 0.0))
                dW = np.sum(dw, axis=0)
                Wc = Wsum[..., None]
                dE = (np.sum(sel(wt[..., None] * E[qj, qi]), axis=0) + np.sum(sel(dw[..., None] * np.abs(eq - ebar[None])), axis=0)
                      + (T + 1) * U * np.sum(sel(wt[..., None] * np.abs(eq)), axis=0) + T * ETA) / Wc
                res.update(dW=dW, dE=dE, dg=dg)
                if have_var:
                    WW = Wc * Wc
                    res["dV"] = ((np.sum(sel((wt * wt)[..., None] * D[qj, qi]), axis=0)
                                  + 2 * np.sum(sel(dw[..., None] * np.abs(wt[..., None] * vq - (vbar * Wc)[None])), axis=0)
                                  + ETA * (np.sum(sel(vq), axis=0) + T + vbar)) / WW + ETA)
            return res

        # ---- stage 0: the 2x2 footprint, dj outer, di inner (the order is immaterial here)
        DI, DJ = np.meshgrid(np.arange(2), np.arange(2))
        DI, DJ = DI.ravel()[:, None, None], DJ.ravel()[:, None, None]
        bx, by = np.where(DI == 1, FX[None], 1.0 - FX[None]), np.where(DJ == 1, FY[None], 1.0 - FY[None])
        dbx, dby = tau * U * np.where(DI == 1, FX[None], 1.0), tau * U * np.where(DJ == 1, FY[None], 1.0)
        b0 = bx * by
        db0 = by * dbx + bx * dby + U * b0
        s0 = taps(I0[None] + DI, J0[None] + DJ, b0, db0, 4)
        if detail is not None:
            detail.update(g0=s0["g"], accepted0=s0["active"])
        # ---- stage 1: the 4x4 footprint, b = 1
        if mis("stage1_3x3_about_nearest"):
            DI, DJ = np.meshgrid(np.arange(-1, 2), np.arange(-1, 2))
            DI, DJ = DI.ravel()[:, None, None], DJ.ravel()[:, None, None]
            I1, J1 = NX[None] + DI, NY[None] + DJ
        else:
            DI, DJ = np.meshgrid(np.arange(-1, 3), np.arange(-1, 3))
            DI, DJ = DI.ravel()[:, None, None], DJ.ravel()[:, None, None]
            I1, J1 = I0[None] + DI, J0[None] + DJ
        b1 = np.ones(I1.shape)
        if mis("stage1_keeps_bilinear"):  # a tent of the footprint's width about the pixel's position
            b1 = np.maximum(1.0 - np.abs(DI - FX[None]) / 2, 0.0) * np.maximum(1.0 - np.abs(DJ - FY[None]) / 2, 0.0)
        s1 = taps(I1, J1, b1, np.zeros(I1.shape), 16)
        # ---- the stages
        in0 = s0["W"] >= WMIN
        in1 = ~in0 & (s1["W"] >= WMIN)
        if mis("stage1_never"):
            in1 = np.zeros_like(in0)
        stage = np.where(in0, 0, np.where(in1, 1, 2)).astype(np.uint8)
        pick = lambda k: np.where(in0[..., None], s0[k], s1[k])  # noqa: E731
        out = pick("ebar") * m_p
        raw = c[NY, NX]
        out2 = (raw / m_lo[NY, NX]) * m_p if mis("stage2_modulated") else raw
        is2 = (stage == 2)[..., None]
        out = np.where(is2, out2, out)
        var = None
        if have_var:
            mm = m_p if mis("variance_modulated_by_m") else m_p * m_p
            var = pick("vbar") * mm
            var2 = _clamp_var(var_in[NY, NX]) if mis("stage2_variance_from_input") else np.full((H, W_, 3), VCAP)
            var = np.where(is2, var2, var)
        # ---- the run with a phase: a sampled pixel whose own tap is accepted with g > 0 passes through
        passed = np.zeros((H, W_), bool)
        own_doubt = np.zeros((H, W_), bool)
        if phase is not None:
            sampled = (FX == 0) & (FY == 0)
            own_g = s0["g"][0]           # tap (i0, j0): di = dj = 0
            own_ok = s0["active"][0]
            passed = sampled & (np.ones_like(sampled) if mis("sample_passes_when_refused") else own_ok & (own_g > 0))
            qi, qj = np.clip(I0, 0, w - 1), np.clip(J0, 0, h - 1)
            out = np.where(passed[..., None], c[qj, qi], out)
            if have_var:
                var = np.where(passed[..., None], _clamp_var(var_in[qj, qi]), var)
            stage = np.where(passed, 0, stage).astype(np.uint8)
            if bound:
                own_dg = s0["dg"][0]
                own_doubt = sampled & own_ok & (own_g <= 2 * own_dg) & (own_dg > 0)
        if not bound:
            return out, var, stage
        # ---- bounds and exclusions
        doubt0 = np.abs(s0["W"] - WMIN) <= 2 * s0["dW"]
        doubt1 = ~in0 & (np.abs(s1["W"] - WMIN) <= 2 * s1["dW"])
        first0 = in0 & (s0["dW"] > 2.0 ** -6 * s0["W"])
        first1 = in1 & (s1["dW"] > 2.0 ** -6 * s1["W"])
        excluded = ((doubt0 | doubt1 | first0 | first1) & ~passed) | own_doubt
        selected = is2[..., 0] | passed
        T = np.where(in0, 4, 16)[..., None]
        cb = 2 * (m_p * pick("dE") + U * np.abs(out))
        cb = np.where(selected[..., None], 0.0, cb)
        vb = None
        if have_var:
            vb = 2 * (m_p * m_p * pick("dV") + (3 * T + 3) * U * np.abs(var))
            vb = np.where(selected[..., None], 0.0, vb)
        return out, cb, var, vb, stage, excluded
