"""DESIGN.md §4.15 in numpy float64, written from the section's text (not from tests/temporal_mirror.cpp): vectorised over the frame
and the taps, dots by `np.sum`, no FMA, no fixed order of summation.  The projection does not use §4.15's cross products at all: it
comes from the camera's definition in §4.10 — the ray through pixel centre (x, y) is look_from + t·((px_origin − look_from) + x·px_du
+ y·px_dv) — by solving the 3×3 system [px_du px_dv a]·(t·x, t·y, t) = P − look_from with `numpy.linalg.solve` on the f64 camera fields.
`TemporalF64` keeps its own state in f64 (the four history records, the previous camera, the has-history flag, and the error bound of
every history value); `step` has the signature of `temporal_ref.Temporal.step`.  A static step is one whose camera equals the stored
one in all 152 bytes.  (What it takes from temporal_ref.py is plain Python and none of the mirror: the parameter defaults, the
camera's twelve doubles and its 152-byte key.)

`misread=` switches in ONE wrong reading of §4.15 (MISREADINGS); the tests require that each is told apart from the mirror.

`step` takes `spp` as one number — this section — or as an (h, w) integer array of per-pixel sample counts: the counts step, §4.23,
whose rules act inside the gather and the blend below and are switched on by the array alone (every `if counts:`).  Their text, bounds
and wrong readings (COUNTS_MISREADINGS) are in tests/temporal_counts_f64.py.

The error bound (first order, carried from step to step, DOUBLED where it is reported or used as a margin).  u = 2^-24; a primed
quantity is the f32 contract's, δq = |q' − q|.

  Projection.  M = [u v a]^-1 and from = look_from are rounded to f32 once: δM_kj <= u|M_kj|, δfrom_j <= u|from_j|.  w_j = P_j − from_j
  is one subtraction of f32 values: δw_j <= u|from_j| + u|w_j|.  A row, α = fma(M_2, w_z, fma(M_1, w_y, M_0·w_x)), has three roundings,
  each at most u times a partial sum that Σ_j |M_j||w_j| dominates.  Together

      δα <= Σ_j (δM_j|w_j| + |M_j|δw_j) + 3u·Σ_j |M_j||w_j|  =  u·Σ_j |M_kj|·(5|w_j| + |from_j|)  =: e_k        (k = 0, 1, 2 for α, β, γ)

  plus this module's own f64 error, 8·2^-53·cond([u v a])·|value|, which is far below e_k for any sane camera but is carried.
  x = α/γ is one rounded divide:  δx <= (e_0 + |x|·e_2)/(γ − e_2) + u|x|,  δy likewise.  (The denominator is the far end of the
  mean-value interval, which makes the expression rigorous up to u² wherever γ > e_2.)

  Weights.  x0 = floor(x), fx = x − x0 (exact for x >= 0, one rounding below), 1 − fx one rounding: as functions of x the two weights
  of an axis are the hat function b_i(x) = max(0, 1 − |x − (x0 + i)|), which is 1-Lipschitz, so δb_i <= δx + 2u, and
  b = b_i·b_j is one product: δb <= b_i δb_j + b_j δb_i + δb_i δb_j + u·b  (the issue's |δb| <= |δfx| + |δfy| plus roundings, kept tight).
  INTEGER POSITIONS ARE BOUNDED THROUGH CONTINUITY, NOT EXCLUDED: if x lies within 2δx of an integer, the f32 run may take its
  four taps one pixel over.  The hat functions say what that does: the tap that f64 does not visit has b = 0 here and at most
  δb_i there, and the tap f64 visits with b = 0 drops out.  So the reference evaluates a 4×4 neighbourhood, i, j ∈ {−1, 0, 1, 2}:
  the outer taps carry b = 0 and a δb that is non-zero only when x (or y) is within the margin of the integer — they add nothing to
  the value, they add δb·|c_q − h| to the bound, and their acceptance decisions count for the exclusion below.

  History.  h = H/B, H = Σ b_q c_q over accepted taps, B = Σ b_q.  With c'_q = c_q + δc_q, δc_q <= E_q (the history's own bound, kept in
  the state), and since Σ b_q (c_q − h) = 0:

      δh <= Σ b_q E_q / B  +  Σ δb_q |c_q − h| / B  +  8u·Σ b_q |c_q| / B        (four FMAs into H, three adds into B, one divide)

  and the same for hv (with the variance's E) and hN (with the length's E).  δB <= Σ δb_q + 3u·B.  A STATIC step's one tap has
  b = 1: B = 1 and every mean is fma(1, x, 0) / 1 = x in any order of the operations, so the last term is 0 there (§4.23 (b)).

  Blend.  spp is exact.  Ns = hN + spp: δNs <= δhN + u·Ns.  a0 = spp/Ns: δa0 <= a0·δNs/Ns + u·a0.  al = max(a0, am): δal <= δa0.
  c_out = fma(al, c − h, h) = al·c + (1 − al)·h with the difference rounded first:
      δc_out <= (1 − al)·δh + |c − h|·δal + al·u·|c − h| + u·|c_out|.
  k = 1 − al: δk <= δal + u·k;  δ(al²) <= 2al·δal + u·al²;  δ(k²) <= 2k·δk + u·k²;
      δv_out <= s·δ(al²) + hv·δ(k²) + k²·δhv + u·k²·hv + u·v_out;      δN_out <= δNs   (min is 1-Lipschitz).
  A pixel without history copies its inputs by selection: E = 0.  The clamp of the input variance acts on values both runs hold
  exactly, and `!(s < 2^32) ? 2^32 : s` is the identity at its own border: it has margin 0 and excludes nothing.

What is dropped is second order (products of two δ), so the reported bound is 2·E, and every decision margin is 2·(its δ).

`excluded` (bound=True).  A hit pixel of a step that reads history is excluded when one of its decisions lies within the doubled
propagated error of its border — γ > 0 (e_2); x > −1, x < W, y > −1, y < H (δx, δy); for a tap that is inside, of the same index, and
has b > 0 or δb > 0: dot(n_prev, n) >= cm (3u·Σ|n_i n'_i|) and dot(d, d) <= lim (5u·dd + r2·(2Σ|w_j|δw_j + 3u·ww) + u·lim);
B >= 2^-6 (δB); a0 < am (δa0); Ns > nm (δNs) — or when an accepted tap with b > 0 or δb > 0 reads a history pixel that was excluded at
the previous step (the taint follows the taps; a static step's only tap is the pixel itself, so it spreads none)."""
import numpy as np

from temporal_ref import DEFAULTS, camera_fields, camera_key

U = 2.0 ** -24
VCAP = 2.0 ** 32
BMIN = 2.0 ** -6
MISREADINGS = ("project_with_current_camera", "matrix_transposed", "pixel_centres_at_half", "from_of_current_camera",
               "distance_absolute", "normal_test_abs", "refused_tap_in_B", "no_divide_by_B", "nearest_tap", "variance_b_squared",
               "variance_linear_alpha", "alpha_by_steps", "length_of_nearest_tap", "clamp_length_before_alpha",
               "alpha_min_is_a_ceiling", "background_takes_history", "history_stores_input", "outside_tap_clamped_in")
# Wrong readings of §4.23 (the counts step), switched in like the others; tests/temporal_counts_f64.py lists and explains them.
COUNTS_MISREADINGS = ("zero_length_record_accepted", "zero_length_tap_in_B", "static_tap_exempt_from_length_test",
                      "alpha_min_applied_at_zero_count", "zero_count_takes_input", "zero_count_resets_length",
                      "length_uncapped_at_zero_count", "variance_from_input_at_zero_count", "count_shared_over_the_frame",
                      "background_keeps_history")


def camera_system(cam):
    """(look_from (3,), A (3, 3)) with A's columns px_du, px_dv, px_origin − look_from: A·(t·x, t·y, t) = P − look_from (§4.10)."""
    f = camera_fields(cam).reshape(4, 3)
    lf, u, v, po = f
    A = np.stack([u, v, po - lf], axis=1)
    with np.errstate(all="ignore"):
        det = np.linalg.det(A) if np.isfinite(A).all() and np.isfinite(lf).all() else np.nan
    if not np.isfinite(det) or det == 0:
        raise ValueError("camera: det is 0 or not finite")
    return lf, A


def project(lf, A, P, half=False):
    """The §4.10 camera (look_from `lf`, system `A`) seen from points P (..., 3): x, y, γ (= the ray parameter t) and the bounds
    δx, δy, e_γ of the module docstring on what the f32 contract computes for the same points."""
    shape = P.shape[:-1]
    W = (P - lf).reshape(-1, 3)
    with np.errstate(all="ignore"):
        sol = np.linalg.solve(A, W.T).T
        al, be, ga = sol[:, 0], sol[:, 1], sol[:, 2]
        x, y = al / ga, be / ga
        M = np.abs(np.linalg.inv(A))
        load = 5 * np.abs(W) + np.abs(lf)[None]
        own = 8 * 2.0 ** -53 * np.linalg.cond(A)
        e = U * load @ M.T + own * np.abs(sol)
        den = np.where(ga - e[:, 2] > 0, ga - e[:, 2], np.nan)
        dx = (e[:, 0] + np.abs(x) * e[:, 2]) / den + U * np.abs(x)
        dy = (e[:, 1] + np.abs(y) * e[:, 2]) / den + U * np.abs(y)
        dx, dy = np.where(np.isnan(dx), np.inf, dx), np.where(np.isnan(dy), np.inf, dy)
    if half:
        x, y = x - 0.5, y - 0.5
    return tuple(a.reshape(shape) for a in (x, y, ga, dx, dy, e[:, 2]))


class TemporalF64:
    def __init__(self, width, height, misread=None):
        assert misread is None or misread in MISREADINGS + COUNTS_MISREADINGS, misread
        self.width, self.height, self.misread = width, height, misread
        self.has_history = False
        self.key = self.cam = None
        self.last_static = None
        self.last_passthrough = None  # (h, w) bool: the pixels whose outputs the last step took from its inputs by selection
        self.taps = None  # the per-tap quantities of the last step that read history (see _blend)
        self.hist = None  # dict: c, v (h, w, 3); N, K (h, w); n, P (h, w, 3); id (h, w); Ec, Ev (h, w, 3); EN (h, w); excluded (h, w)

    def reset(self):
        self.has_history = False

    def step(self, rgb, var_rgb, index, normal, point, camera, spp, length=True, bound=False, **params):
        """Returns (colour (h, w, 3), variance (h, w, 3)[, length (h, w)]) in float64; with bound=True two more entries: the bounds
        (for colour, variance and length, shaped like them) and the `excluded` mask (h, w).  `spp` is one number (§4.15) or an (h, w)
        array of non-negative integers, one sample count per pixel: the counts step, §4.23 (tests/temporal_counts_f64.py)."""
        assert not (bound and self.misread), "the bound belongs to the reference as written"
        mis = lambda name: self.misread == name  # noqa: E731
        prm = {**DEFAULTS, **params}
        h, w = self.height, self.width
        f32 = lambda z: np.float64(np.float32(z))  # noqa: E731
        with np.errstate(over="ignore"):
            am, nm, cm = f32(prm["alpha_min"]), f32(prm["n_max"]), f32(prm["normal_cos_min"])
            r = np.float32(prm["max_rel_dist"])
            r2 = np.float64(r * r)  # an f32 product
        counts = np.ndim(spp) != 0
        if counts:
            spp = np.asarray(spp)
            assert spp.shape == (h, w) and spp.dtype.kind in "iu" and (spp >= 0).all() and (spp <= 2 ** 24).all(), (spp.shape, spp.dtype)
            spp = spp.astype(np.float64)  # n = f32(count), exact up to 2^24
            if mis("count_shared_over_the_frame"):
                counts, spp = False, float(spp.mean())
        else:
            spp = float(spp)
        c = np.asarray(rgb, np.float64).reshape(h, w, 3)
        s = np.asarray(var_rgb, np.float64).reshape(h, w, 3)
        n = np.asarray(normal, np.float64).reshape(h, w, 3)
        P = np.asarray(point, np.float64).reshape(h, w, 3)
        idx = np.asarray(index).reshape(h, w).astype(np.int64)
        with np.errstate(invalid="ignore"):
            s = np.where(~(s < VCAP), VCAP, np.where(s > 0, s, 0.0))
        lf, A = camera_system(camera)
        key = camera_key(camera)
        static = self.has_history and key == self.key
        had = self.has_history
        hit = idx >= 0
        zero3, zero1 = np.zeros((h, w, 3)), np.zeros((h, w))
        has = np.zeros((h, w), bool)
        excluded = np.zeros((h, w), bool)
        c_out, v_out, N_out, K_out = c.copy(), s.copy(), (spp.copy() if counts else np.full((h, w), spp)), np.ones((h, w))
        Ec, Ev, EN = zero3.copy(), zero3.copy(), zero1.copy()
        if self.has_history:
            with np.errstate(all="ignore"):
                has, excluded, (c_b, v_b, N_b, K_b), (Ec_b, Ev_b, EN_b) = self._blend(
                    mis, static, c, s, n, P, idx, hit, lf, A, spp, am, nm, cm, r2, counts)
            sel = lambda m, a, b: np.where(m[..., None] if a.ndim == 3 else m, a, b)  # noqa: E731
            c_out, v_out, N_out, K_out = sel(has, c_b, c_out), sel(has, v_b, v_out), sel(has, N_b, N_out), sel(has, K_b, K_out)
            Ec, Ev, EN = sel(has, Ec_b, Ec), sel(has, Ev_b, Ev), sel(has, EN_b, EN)
        self.hist = dict(c=c.copy() if mis("history_stores_input") else c_out, v=v_out, N=N_out, K=K_out, n=n, P=P, id=idx,
                         Ec=Ec, Ev=Ev, EN=EN, excluded=excluded)
        self.has_history, self.key, self.cam, self.last_static = True, key, (lf, A), static
        self.last_passthrough = ~has & ~excluded
        self.last_had = had
        res = (c_out, v_out) + ((N_out,) if length else ())
        if bound:
            res += ((2 * Ec, 2 * Ev) + ((2 * EN,) if length else ()), excluded)
        return res

    # ---- steps 2-4 for a handle that has history ------------------------------------------------------------------------------
    def _blend(self, mis, static, c, s, n, P, idx, hit, lf, A, spp, am, nm, cm, r2, counts=False):
        h, w = self.height, self.width
        H = self.hist
        gy, gx = np.mgrid[0:h, 0:w]
        plf, pA = self.cam
        fr = lf if (mis("from_of_current_camera") or mis("project_with_current_camera")) else plf
        Wv = P - fr
        ww = np.sum(Wv * Wv, axis=-1)
        lim = np.full((h, w), r2) if mis("distance_absolute") else r2 * ww
        dw = U * (np.abs(fr) + np.abs(Wv))
        dlim = r2 * (2 * np.sum(np.abs(Wv) * dw, axis=-1) + 3 * U * ww) + U * lim
        near = np.zeros((h, w), bool)  # a decision within its margin
        if static:
            ok = hit.copy()
            qx, qy = gx[None], gy[None]
            b, db = np.ones((1, h, w)), np.zeros((1, h, w))
            inside = np.ones((1, h, w), bool)
        else:
            sysA = A if mis("project_with_current_camera") else pA
            if mis("matrix_transposed"):
                sysA = sysA.T
            x, y, ga, dx, dy, dga = project(fr, sysA, P, half=mis("pixel_centres_at_half"))
            ok = hit & (ga > 0) & (x > -1) & (x < w) & (y > -1) & (y < h)
            gnear = np.abs(ga) <= 2 * dga
            fnear = (ga > 0) & ((np.abs(x + 1) <= 2 * dx) | (np.abs(x - w) <= 2 * dx) | (np.abs(y + 1) <= 2 * dy) | (np.abs(y - h) <= 2 * dy))
            near |= hit & (gnear | fnear)
            x, y = np.where(ok, x, 0.0), np.where(ok, y, 0.0)
            dx, dy = np.where(ok, dx, 0.0), np.where(ok, dy, 0.0)
            x0, y0 = np.floor(x), np.floor(y)
            off = np.arange(-1, 3, dtype=np.float64)
            def axis(t, t0, dt):  # noqa: E306
                dist = np.abs(t[None] - (t0[None] + off[:, None, None]))
                if mis("nearest_tap"):
                    return (dist <= 0.5) & (np.cumsum(dist <= 0.5, axis=0) == 1), np.zeros_like(dist)
                return np.maximum(0.0, 1.0 - dist), np.where(dist <= 1 + 2 * dt[None], dt[None] + 2 * U, 0.0)
            bx, dbx = axis(x, x0, dx)
            by, dby = axis(y, y0, dy)
            bx, by = bx.astype(np.float64), by.astype(np.float64)
            b = (by[:, None] * bx[None]).reshape(16, h, w)  # j outer, i inner (the order is immaterial here)
            db = (by[:, None] * dbx[None] + dby[:, None] * bx[None] + dby[:, None] * dbx[None]).reshape(16, h, w) + U * b
            qx = (x0[None, None] + off[None, :, None, None] + 0 * off[:, None, None, None]).reshape(16, h, w).astype(np.int64)
            qy = (y0[None, None] + off[:, None, None, None] + 0 * off[None, :, None, None]).reshape(16, h, w).astype(np.int64)
            inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
            qx, qy = np.clip(qx, 0, w - 1), np.clip(qy, 0, h - 1)
            if mis("outside_tap_clamped_in"):
                inside = np.ones_like(inside)
        rel = (b > 0) | (db > 0)
        nq, Pq = H["n"][qy, qx], H["P"][qy, qx]
        same = inside & (H["id"][qy, qx] == idx[None]) & ok[None]
        dn = np.sum(nq * n[None], axis=-1)
        ddn = 3 * U * np.sum(np.abs(nq * n[None]), axis=-1)
        d = Pq - P[None]
        dd = np.sum(d * d, axis=-1)
        acc = same & ((np.abs(dn) if mis("normal_test_abs") else dn) >= cm) & (dd <= lim[None])
        tnear = same & rel & ((np.abs(dn - cm) <= 2 * ddn) | (np.abs(dd - lim[None]) <= 2 * (5 * U * dd + dlim[None])))
        self.length_near = np.zeros((h, w), bool)
        live = acc  # (the taps §4.15's tests accept)
        if counts:
            # §4.23 rule 1: a record of length 0 holds no samples and is refused — the static step's one tap too.  A length is 0
            # exactly (rule 2 stored a count of 0) or positive; the decision gets the margin every other one has.
            Nq, ENq = H["N"][qy, qx], H["EN"][qy, qx]
            lnear = same & rel & (Nq > 0) & (Nq <= 2 * ENq)
            self.length_near = lnear.any(axis=0)
            tnear = tnear | lnear
            if not (mis("zero_length_record_accepted") or (static and mis("static_tap_exempt_from_length_test"))):
                acc = acc & (Nq > 0)
            self.refused_empty = (live & ~acc & (b > 0)).any(axis=0)  # a tap with b > 0 that only rule 1 refuses
        near |= tnear.any(axis=0)
        taint = (acc & rel & H["excluded"][qy, qx]).any(axis=0)

        ba = np.where(acc, b, 0.0)
        dba = np.where(acc, db, 0.0)
        B = np.sum(np.where(inside & ok[None], b, 0.0), axis=0) if mis("refused_tap_in_B") else np.sum(ba, axis=0)
        if mis("zero_length_tap_in_B"):
            B = np.sum(np.where(live, b, 0.0), axis=0)
        dB = np.sum(dba, axis=0) + 3 * U * B
        near |= ok & (np.abs(B - BMIN) <= 2 * dB)
        has = ok & (B >= BMIN)
        div = np.ones((h, w)) if mis("no_divide_by_B") else np.where(has, B, 1.0)

        def gather(val, E, weight=ba, norm=div):
            """h = Σ b v_q / B over accepted taps and its bound; val (h, w[, 3])."""
            three = val.ndim == 3
            ex = (lambda z: z[..., None]) if three else (lambda z: z)
            # the records are SELECTED before they meet a weight: a refused record may hold a NaN (§4.23), and 0·NaN is NaN
            used = ex((weight != 0) | (ba != 0) | (dba != 0))
            vq, Eq = np.where(used, val[qy, qx], 0.0), np.where(used, E[qy, qx], 0.0)
            hh = np.sum(ex(weight) * vq, axis=0) / ex(norm)
            Eh = (np.sum(ex(ba) * Eq, axis=0) + np.sum(ex(dba) * np.abs(vq - hh[None]), axis=0)
                  + rnd * np.sum(ex(ba) * np.abs(vq), axis=0)) / ex(div)
            return hh, Eh

        # A static step's one tap has b = 1, so B = 1 and every mean is fma(1, x, 0) / 1 = x, whatever the order of the operations
        # (§4.23 (b)): the gather rounds nothing there and δh is the record's own E.  (Without this a kept W2 = 1 of a first frame,
        # with w2_max = 1, would sit within a margin of 8u that no f32 run can use.)
        rnd = 0.0 if static else 8 * U

        hc, Ehc = gather(H["c"], H["Ec"])
        if mis("variance_b_squared"):
            hv, Ehv = gather(H["v"], H["Ev"], weight=ba * ba, norm=div * div)
        else:
            hv, Ehv = gather(H["v"], H["Ev"])
        hN, EhN = gather(H["N"], H["EN"])
        hK, _ = gather(H["K"], H["EN"])
        if mis("length_of_nearest_tap"):
            best = np.argmax(ba, axis=0)
            hN = np.take_along_axis(H["N"][qy, qx], best[None], axis=0)[0]
        if mis("background_takes_history") or mis("background_keeps_history"):
            both = ~hit & (H["id"] < 0)
            e3 = both[..., None]
            hc, hv, hN, hK = np.where(e3, H["c"], hc), np.where(e3, H["v"], hv), np.where(both, H["N"], hN), np.where(both, H["K"], hK)
            has = has | both

        Ns = hN + spp
        dNs = EhN + U * Ns
        if mis("clamp_length_before_alpha"):
            Ns = np.where(Ns > nm, nm, Ns)
        a0 = 1.0 / (hK + 1.0) if mis("alpha_by_steps") else spp / Ns
        da0 = a0 * dNs / Ns + U * a0
        al = np.where(a0 > am, am, a0) if mis("alpha_min_is_a_ceiling") else np.where(a0 < am, am, a0)
        sampled = np.ones((h, w), bool)
        if counts:
            # §4.23 rule 4: history found and n = 0.  al = 0 by selection — a0 < am is not decided and has no margin — and the input
            # is never read: c_out = h (δh), v_out = hv (δhv), N_out = hN > nm ? nm : hN (δhN, the margin on nm is 2·δhN).
            sampled = spp > 0
            dNs = np.where(sampled, dNs, EhN)
            if not mis("alpha_min_applied_at_zero_count"):
                al, da0 = np.where(sampled, al, 0.0), np.where(sampled, da0, 0.0)
                near |= has & np.where(sampled, np.abs(a0 - am) <= 2 * da0, False)
            else:
                near |= has & (np.abs(a0 - am) <= 2 * da0)
            near |= has & (np.abs(Ns - nm) <= 2 * dNs)
        else:
            near |= has & ((np.abs(a0 - am) <= 2 * da0) | (np.abs(Ns - nm) <= 2 * dNs))
        k = 1.0 - al
        a3, k3 = al[..., None], k[..., None]
        diff = c - hc
        c_b = a3 * diff + hc
        Ec = k3 * Ehc + np.abs(diff) * da0[..., None] + a3 * U * np.abs(diff) + U * np.abs(c_b)
        dk = da0 + U * k
        da2, dk2 = 2 * al * da0 + U * al * al, 2 * k * dk + U * k * k
        if mis("variance_linear_alpha"):
            v_b = a3 * s + k3 * hv
        else:
            v_b = a3 * a3 * s + k3 * k3 * hv
        Ev = s * da2[..., None] + hv * dk2[..., None] + k3 * k3 * Ehv + U * k3 * k3 * hv + U * v_b
        N_b = np.where(Ns > nm, nm, Ns)
        if counts:
            kept = ~sampled  # rule 4, by selection on the VALUE: the input of such a pixel may be a NaN
            k3 = kept[..., None]
            if not (mis("alpha_min_applied_at_zero_count") or mis("zero_count_takes_input")):
                c_b, Ec = np.where(k3, hc, c_b), np.where(k3, Ehc, Ec)
            if mis("zero_count_takes_input"):
                c_b, Ec = np.where(k3, c, c_b), np.where(k3, 0.0, Ec)
            if mis("zero_count_takes_input") or mis("variance_from_input_at_zero_count"):
                v_b, Ev = np.where(k3, s, v_b), np.where(k3, 0.0, Ev)
            elif not mis("alpha_min_applied_at_zero_count"):
                v_b, Ev = np.where(k3, hv, v_b), np.where(k3, Ehv, Ev)
            if mis("zero_count_resets_length"):
                N_b = np.where(kept, 0.0, N_b)
            if mis("length_uncapped_at_zero_count"):
                N_b = np.where(kept, hN, N_b)
        excluded = hit & (near | (has & taint))
        # what a step that rides the same taps needs (tests/temporal_moments_f64.py); nothing above depends on it
        self.taps = dict(b=b, db=db, ba=ba, dba=dba, qy=qy, qx=qx, inside=inside, ok=ok, div=div, has=has, al=al, da0=da0, hc=hc,
                         near=near, taint=taint, gather=gather, sampled=sampled, acc=acc)
        return has, excluded, (c_b, v_b, N_b, hK + 1.0), (Ec, Ev, dNs)


def within_bound(got, ref, hit, what, cap=0.02):
    """Holds one step's f32 outputs `got` (colour, variance[, length]) to `ref`, what `step(..., bound=True)` returned for the same
    inputs: at most `cap` of the hit pixels excluded, and every value of every other pixel within its bound.  Returns the largest
    |difference| / bound per output (0 where both are 0) and the excluded share."""
    vals, (bnds, ex) = ref[:-2], ref[-2:]
    assert len(got) == len(vals) == len(bnds), what
    share = float(ex[hit].sum()) / max(int(hit.sum()), 1)
    assert not ex[~hit].any() and share <= cap, f"{what}: {int(ex.sum())} of {int(hit.sum())} hit pixels excluded (cap {cap})"
    ratios = []
    for name, g, x, b in zip(("colour", "variance", "length"), got, vals, bnds):
        keep = ~ex if g.ndim == 2 else np.broadcast_to(~ex[..., None], g.shape)
        d = np.abs(np.asarray(g, np.float64) - x)
        bad = np.argwhere(keep & ~(d <= b))
        assert len(bad) == 0, f"{what} {name}: {len(bad)} values outside the bound; first at {bad[:3].tolist()}: " \
                              f"{[(float(g[tuple(i)]), float(x[tuple(i)]), float(b[tuple(i)])) for i in bad[:3]]}"
        with np.errstate(all="ignore"):
            ratios.append(float(np.where(d == 0, 0.0, d / b)[keep].max()) if keep.any() else 0.0)
    return ratios, share
