"""DESIGN.md §4.26 in numpy float64, written from the section: the weights, the sums, the divide and the clamp of the cubic path, and
around them as much of §4.15 as a pixel needs (projection, acceptance, the bilinear means, the blend) — so that a MISREADING of the
section can be switched on and shown to be caught.

The bound (first order in u = 2^-24; every |w| <= 1, Σ|b| <= 1.5625).  A weight is four rounded operations on magnitudes <= 2.5, so
|δw| <= 8u absolutely (relative to a small w it is unbounded, which is why Σ|c| appears below and not only Σ|b||c|).
b = wx·wy: |δb| <= |wx||δwy| + |wy||δwx| + u|b| <= 17u.  C = Σ fma(b, c, C) over 16 taps: |δC| <= Σ|δb||c| + 16u·Σ|b||c|
<= 17u·T + 16u·S with S = Σ|b||c| and T = Σ|c| over the sixteen taps.  W likewise: |δW| <= 16·17u + 16u·1.5625 < 297u, and W = 1
in exact arithmetic.  hc = C / W: |δhc| <= |δC| + |hc||δW| + u|hc| with |hc| <= S: E_h = u·(17·T + 314·S).  The clamp's limits are
taps, which carry no error, and clamping is 1-Lipschitz, so the clamped h inherits E_h.  The blend out = fma(al, c − h, h): al is
a quotient of the bilinear length (B = 1 ± 4u here, HN / B and spp / Ns: |δal| <= 10u), so
|δout| <= E_h + 12u·(|c| + |h|); the tests allow BOUND = E_h + 16u·(|c| + |h|) per channel.

On a sequence only the pixels the mirror TOOK are compared (all sixteen taps accepted, so no acceptance decision is re-made in
f64), and of those only the ones whose projected position lies more than 1e-4 from a pixel boundary (f32 and f64 then floor
alike).  Misreadings that change WHICH pixels are taken are caught on the hand cases, whose exact cameras and far-from-threshold
guides make every decision the same in f64.

SWITCHES names the misreadings; `caught_by(switch)` lists the hand cases it fails and the sequences on which it leaves the bound."""
import numpy as np

import temporal_cases
import temporal_cubic_cases as cases
import temporal_cubic_ref as ref

U = 2.0 ** -24
SWITCHES = {
    "a=-0.75": "the kernel parameter of the cubic is −0.75 (Mitchell-style sharpening) and not Catmull-Rom's −0.5",
    "a=-1": "the kernel parameter is −1",
    "no-divide": "hc = C, not C / W (W = 1 + O(u): held in f32 by the mirror on the case 'divide', see caught_by)",
    "clamp-16": "the clamp's range is taken over all sixteen taps",
    "no-clamp": "no clamp",
    "cubic-length": "the history length is resampled by the sixteen taps too",
    "cubic-variance": "the variance is resampled by the sixteen taps too",
    "refused-is-no-history": "a refused outer tap means the pixel has no history",
    "inside-only": "the sixteen taps need only lie inside the frame: acceptance is asked of the inner four alone",
}


def weights(f, a=-0.5):
    """Keys' cubic convolution weights with parameter a; a = −0.5 is §4.26's."""
    return np.array([a * f * (1 - f) ** 2, (a + 2) * f ** 3 - (a + 3) * f ** 2 + 1, -(a + 2) * f ** 3 + (2 * a + 3) * f ** 2 - a * f,
                     a * f * f * (1 - f)], np.float64)


def section_weights(f):
    """§4.26's own Horner forms, in f64."""
    return np.array([f * (f * (-0.5 * f + 1) - 0.5), f * f * (1.5 * f - 2.5) + 1, f * (f * (-1.5 * f + 2) + 0.5), f * f * (0.5 * f - 0.5)], np.float64)


def pixel(state, M, fr, frame, py, px, spp, prm, switch=None, trust_taken=False):
    """One pixel of a moved plain step in f64: (colour (3,), variance (3,), length, taken, E_h + blend slack per channel (3,)), or None
    where the position is too near a pixel boundary to floor alike in f32."""
    c_h, v_h, g_h, p_h = (a.astype(np.float64) for a in state)
    idx_h = state[2][..., 3].view(np.int32)
    h_, w_ = idx_h.shape
    c, s = frame["rgb"][py, px].astype(np.float64), np.clip(np.nan_to_num(frame["var"][py, px].astype(np.float64), nan=2.0 ** 32), 0, 2.0 ** 32)
    n, P, pid = frame["normal"][py, px].astype(np.float64), frame["point"][py, px].astype(np.float64), int(frame["index"][py, px])
    none = (c, s, float(spp), 0, np.zeros(3))
    if pid < 0:
        return none
    wv = P - fr.astype(np.float64)
    lim = float(np.float32(prm["max_rel_dist"])) ** 2 * (wv @ wv)
    al, be, ga = (M.astype(np.float64).reshape(3, 3) @ wv)
    if not ga > 0:
        return none
    x, y = al / ga, be / ga
    if not (-1 < x < w_ and -1 < y < h_):
        return none
    x0, y0 = int(np.floor(x)), int(np.floor(y))
    fx, fy = x - x0, y - y0
    if any(0 < min(f, 1 - f) < 1e-4 for f in (fx, fy)):  # (exactly on a boundary — the exact cameras — floors alike)
        return None

    def accepts(qx, qy):
        if not (0 <= qx < w_ and 0 <= qy < h_):
            return False
        if trust_taken:
            return True
        d = p_h[qy, qx, :3] - P
        return idx_h[qy, qx] == pid and g_h[qy, qx, :3] @ n >= float(np.float32(prm["normal_cos_min"])) and d @ d <= lim

    B, H, Hv, HN = 0.0, np.zeros(3), np.zeros(3), 0.0
    for j in (0, 1):
        for i in (0, 1):
            if accepts(x0 + i, y0 + j):
                b = (fx if i else 1 - fx) * (fy if j else 1 - fy)
                B, H, Hv, HN = B + b, H + b * c_h[y0 + j, x0 + i, :3], Hv + b * v_h[y0 + j, x0 + i, :3], HN + b * c_h[y0 + j, x0 + i, 3]
    if not B >= 2.0 ** -6:
        return none
    h, hv, hN = H / B, Hv / B, HN / B
    taken, E = 0, np.zeros(3)
    inside = x0 >= 1 and x0 + 2 < w_ and y0 >= 1 and y0 + 2 < h_
    need = [(i, j) for j in (-1, 0, 1, 2) for i in (-1, 0, 1, 2)]
    if switch == "inside-only":
        need = [(i, j) for j in (0, 1) for i in (0, 1)]
    ok = inside and all(accepts(x0 + i, y0 + j) for i, j in need)
    if inside and not ok and switch == "refused-is-no-history":
        return none
    if ok:
        a = {"a=-0.75": -0.75, "a=-1": -1.0}.get(switch)
        wx, wy = (section_weights(fx), section_weights(fy)) if a is None else (weights(fx, a), weights(fy, a))
        win = c_h[y0 - 1:y0 + 3, x0 - 1:x0 + 3]
        b = np.outer(wy, wx)
        W = b.sum()
        C = np.tensordot(b, win, axes=([0, 1], [0, 1]))
        hc = C / W
        rng = win[..., :3].reshape(16, 3) if switch == "clamp-16" else win[1:3, 1:3, :3].reshape(4, 3)
        h = hc[:3] if switch == "no-clamp" else np.clip(hc[:3], rng.min(0), rng.max(0))
        if switch == "cubic-length":
            hN = hc[3]
        if switch == "cubic-variance":
            hv = np.tensordot(b, v_h[y0 - 1:y0 + 3, x0 - 1:x0 + 3, :3], axes=([0, 1], [0, 1])) / W
        S, T = np.tensordot(np.abs(b), np.abs(win[..., :3]), axes=([0, 1], [0, 1])), np.abs(win[..., :3]).sum((0, 1))
        E = U * (17 * T + 314 * S)
        taken = 1
    Ns = hN + spp
    a0 = spp / Ns
    alpha = max(a0, float(np.float32(prm["alpha_min"])))
    k = 1 - alpha
    out = alpha * (c - h) + h
    return out, alpha * alpha * s + k * k * hv, min(Ns, float(np.float32(prm["n_max"]))), taken, E + 16 * U * (np.abs(c) + np.abs(h))


def sequence(name, w, h):
    if name == "blocks":
        return cases.block_sequence(w, h, 11 * w + h)
    return temporal_cases.moving_sequence(w, h, 3 * w + h)


def check_sequence(name, w, h, switch=None):
    """The worst |mirror − f64| / BOUND over the taken pixels of the sequence's moved steps (0 where none was taken)."""
    m = ref.Temporal(w, h, "cubic")
    worst, seen = 0.0, 0
    for f in sequence(name, w, h):
        state, M, fr, had = m.state(), m.M.copy(), m.fr.copy(), m.has_history
        spp = f.get("spp", 8)
        out = m.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], spp)
        if not had or m.last_static:
            continue
        for py, px in np.argwhere(m.taken == 1):
            r = pixel(state, M, fr, f, py, px, spp, ref.DEFAULTS, switch, trust_taken=True)
            if r is None:
                continue
            seen += 1
            worst = max(worst, float((np.abs(out[0][py, px] - r[0]) / r[4]).max()))
            if switch in ("cubic-length", "cubic-variance"):
                worst = max(worst, abs(out[2][py, px] - r[2]) / (64 * U * r[2]))
                worst = max(worst, float((np.abs(out[1][py, px] - r[1]) / (64 * U * np.abs(r[1]) + 1e-30))[np.isfinite(r[1]) & (r[1] < 2.0 ** 31)].max(initial=0)))
    assert seen >= 10, (name, seen)
    return worst


def check_case(case, switch=None):
    """A hand case's last step in f64 under `switch` against the case's rational expectations: the names of what differs."""
    h_, w_ = case.steps[0].index.shape
    m = ref.Temporal(w_, h_, "cubic")
    for s in case.steps[:-1]:
        m.step(s.rgb, s.var, s.index, s.normal, s.point, s.camera, s.spp, **s.params)
    state, M, fr = m.state(), m.M.copy(), m.fr.copy()
    s = case.steps[-1]
    frame = dict(rgb=s.rgb, var=s.var, index=s.index, normal=s.normal, point=s.point)
    bad = []
    for p, (cv, vv, N) in case.want.items():
        r = pixel(state, M, fr, frame, p[0], p[1], s.spp, {**ref.DEFAULTS, **s.params}, switch)
        tol = r[4] + 1e-12
        if (np.abs(r[0] - [float(x) for x in cv]) > tol).any() or abs(r[2] - float(N)) > 1e-6 * float(N) or \
                (np.abs(r[1] - [float(x) for x in vv]) > 1e-6 * np.array([float(x) for x in vv]) + 1e-12).any():
            bad.append(p)
        if p in case.taken and r[3] != case.taken[p]:
            bad.append(("taken", p))
    for p, t in case.taken.items():
        if p not in case.want:
            r = pixel(state, M, fr, frame, p[0], p[1], s.spp, {**ref.DEFAULTS, **s.params}, switch)
            if r[3] != t:
                bad.append(("taken", p))
    return bad


def caught_by(switch):
    """["case <name>", .., "sequence <name>", ..]: where the misreading shows.  Without a switch the list must be empty."""
    if switch == "no-divide":
        # W = 1 + O(u): the two readings agree far inside any f64 bound, so this one is held in f32.  The mirror runs the case
        # "divide"; the reading is caught if what the mirror returns differs, in bits, from the no-divide value in every channel
        # (and it must equal the divided one, which test_mirror_gives_the_hand_derived_answers[divide] asserts).
        c = cases.divide_case()
        m = ref.Temporal(6, 6, "cubic")
        rgb, _, _ = c.run(m, lambda hd, st: hd.step(st.rgb, st.var, st.index, st.normal, st.point, st.camera, st.spp, **st.params))
        wrong = np.array([float(v) for v in c.without_divide], np.float32)
        return ["case divide"] if (rgb[2, 2].view(np.uint32) != wrong.view(np.uint32)).all() and m.taken[2, 2] == 1 else []
    out = [f"case {c.name}" for c in cases.cases() + [length_case(), variance_case()] if check_case(c, switch)]
    if switch in (None, "a=-0.75", "a=-1", "no-divide", "clamp-16", "no-clamp"):
        out += [f"sequence {n}" for n in ("blocks",) if check_sequence(n, 45, 23, switch) > 1.0]
    return out


def length_case():
    """History LENGTHS that differ by column.  Step 2 looks from cam(−3, 0): the columns x >= 3 find step 1's pixel (y, x − 3) and are
    given its colour again (the mean of two equal colours: exact), N = 8, v = V0/2; the columns x < 3 have no history: their input,
    N = 4, v = V0.  Step 3 looks from cam(−11/4, 1/4): the pixel (2, 2) lay at (2 + 1/4, 2 + 1/4) of step 2: window columns 1 .. 4 with
    lengths (4, 4, 8, 8).  Bilinear: hN = 3/4·4 + 1/4·8 = 5, hv = 3/4·V0 + 1/4·V0/2 = 7/8·V0; a cubic length would be
    (−9·4 + 111·4 + 29·8 − 3·8)/128 = 77/16."""
    from fractions import Fraction as F
    from temporal_cases import V0, blend, cam, col
    Step = cases.CStep

    def second(y, x):
        return cases.quad(y, x - 3) if x >= 3 else cases.quad(y, x)

    steps = [Step(6, 6, cam(0, 0), cases.quad), Step(6, 6, cam(-3, 0), second), Step(6, 6, cam(F(-11, 4), F(1, 4)), 0)]
    win = [[second(y, x) for x in (1, 2, 3, 4)] for y in (1, 2, 3, 4)]
    h = tuple(cases.cubic([[col(v)[ch] for v in row] for row in win], F(1, 4), F(1, 4)) for ch in range(3))
    w = blend(col(0), V0, h, tuple(F(7, 8) * v for v in V0), 5, 4)
    assert w[2] == 9
    return cases.CubicCase("length-bilinear", length_case.__doc__, steps, {(2, 2): w}, {(2, 2): 1})


def variance_case():
    """The clamp-high case with a history VARIANCE that differs by column — (1, 0, 0, 1)·V0 over columns 1 .. 4: the bilinear variance of
    the inner pair is 0, a cubic one would be −V0/8."""
    from fractions import Fraction as F
    from temporal_cases import cam, col
    Step = cases.CStep

    row = {2: 1, 3: 1}
    base = lambda y, x: F(row.get(x, 0))  # noqa: E731
    var = lambda y, x: tuple(float(v) for v in (cases.V0 if x in (1, 4) else (0, 0, 0)))  # noqa: E731
    steps = [Step(6, 6, cam(0, 0), base, var=var), Step(6, 6, cam(F(1, 2), 0), 0, var=(0.0, 0.0, 0.0))]
    return cases.CubicCase("variance-bilinear", variance_case.__doc__, steps, {(2, 2): (tuple(c / 2 for c in col(1)), (0, 0, 0), 8)}, {(2, 2): 1})
