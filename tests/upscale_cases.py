"""Hand cases for guided upscaling with closed-form answers, bit for bit.

Every case is built from LABELS: a full-size and a low-resolution map of surface numbers (-1: background, 0..2: three mutually
perpendicular planes through the origin).  A pixel of plane k gets that plane's normal and a point IN the plane, so between two
pixels of one plane the guide weight is exactly 1 (dot(n, n) = 1; the tap lies in the centre's tangent plane: pl = 0, wz = 1),
between pixels of two planes it is exactly 0 (dot(n_p, n_q) = 0), and background never mixes with a hit.  With dyadic colours,
albedos and variances every product and sum of §4.20 is exact and only the final divide rounds, so the answer is the RATIONAL value

    out = (Σ b·e_q / Σ b)·m_p,   var = (Σ b²·ve_q / (Σ b)²)·m_p²        over the taps of the pixel's own surface,

rounded once — worked out here in Fractions from the labels alone (`expected`), not from any filter code.  A case also names the
closed form the issue states for it, which tests/test_upscale_cpu.py asserts on top."""
from fractions import Fraction as Fr

import numpy as np

from upscale_ref import Guides

NORMALS = {0: (0.0, 0.0, 1.0), 1: (1.0, 0.0, 0.0), 2: (0.0, 1.0, 0.0)}
VCAP = np.float32(4294967296.0)


def _point(label, X, Y):
    """A point of plane `label` for screen position (X, Y): its component along the plane's normal is 0."""
    return {0: (X, Y, 0.0), 1: (0.0, Y, X), 2: (X, 0.0, Y)}[label]


def guides(labels, f_units, albedo=None):
    """Guides for a label map whose pixel (i, j) sits at screen position ((i + 1/2)·f_units, (j + 1/2)·f_units) in full-pixel units.
    Background pixels get what a camera query writes on a miss: index -1, zero normal, point and albedo."""
    labels = np.asarray(labels, dtype=np.int32)
    h, w = labels.shape
    normal, point = np.zeros((h, w, 3), np.float32), np.zeros((h, w, 3), np.float32)
    for j in range(h):
        for i in range(w):
            k = int(labels[j, i])
            if k >= 0:
                normal[j, i] = NORMALS[k]
                point[j, i] = _point(k, (i + 0.5) * f_units, (j + 0.5) * f_units)
    if albedo is not None:
        albedo = np.array(np.broadcast_to(np.asarray(albedo, np.float32), (h, w, 3)))
        albedo[labels < 0] = 0.0
    return Guides(labels, normal, point, albedo)


def _exact32(x):
    """The Fraction x as a float32, which it must be exactly."""
    v = np.float32(float(x))
    assert Fr(float(v)) == x, f"{x} is not a float32: the case is not exact"
    return v


def _round32(x):
    return np.float32(float(x))  # (float(Fraction) rounds correctly to f64; none of the cases' quotients lies near an f32 tie)


def expected(case):
    """(out, var or None, stage) of a case from its labels, in Fractions; pixels outside case['check'] are left 0."""
    f, lab_lo, lab_hi = case["f"], np.asarray(case["labels_lo"]), np.asarray(case["labels_hi"])
    h, w = lab_lo.shape
    H, W = lab_hi.shape
    rgb, var = case["rgb_lo"], case.get("var_lo")
    demod = case.get("flags", 1) & 1
    m_lo = case["g_lo"].albedo if demod else None
    m_hi = case["g_hi"].albedo if demod else None
    lo8 = Fr(1, 256)

    def mod(alb, lab, j, i, c):
        if alb is None or lab[j, i] < 0:
            return Fr(1)
        return max(Fr(float(alb[j, i, c])), lo8)

    out, vout, stage = np.zeros((H, W, 3), np.float32), (np.zeros((H, W, 3), np.float32) if var is not None else None), np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            if "check" in case and not case["check"][y, x]:
                continue
            ax, ay = 2 * x + 1 - f, 2 * y + 1 - f
            i0, j0 = ax // (2 * f), ay // (2 * f)  # (Python's // floors)
            fx, fy = Fr(ax - 2 * f * i0, 2 * f), Fr(ay - 2 * f * j0, 2 * f)
            for st in (0, 1, 2):
                taps = []
                if st == 0:
                    taps = [(i0 + di, j0 + dj, (fx if di else 1 - fx) * (fy if dj else 1 - fy)) for dj in (0, 1) for di in (0, 1)]
                elif st == 1:
                    taps = [(i0 + di, j0 + dj, Fr(1)) for dj in (-1, 0, 1, 2) for di in (-1, 0, 1, 2)]
                taps = [(i, j, b) for i, j, b in taps if 0 <= i < w and 0 <= j < h and b != 0 and lab_lo[j, i] == lab_hi[y, x]]
                Wsum = sum(b for _, _, b in taps)
                if st < 2 and Wsum > 0:
                    _exact32(Wsum)
                    for c in range(3):
                        acc = sum(b * Fr(float(rgb[j, i, c])) / mod(m_lo, lab_lo, j, i, c) for i, j, b in taps)
                        _exact32(acc)
                        mp = mod(m_hi, lab_hi, y, x, c)
                        out[y, x, c] = _exact32(Fr(float(_round32(acc / Wsum))) * mp)
                        if var is not None:
                            V = sum(b * b * Fr(float(var[j, i, c])) / mod(m_lo, lab_lo, j, i, c) ** 2 for i, j, b in taps)
                            _exact32(V), _exact32(Wsum * Wsum)
                            vout[y, x, c] = _exact32(Fr(float(_round32(V / (Wsum * Wsum)))) * mp * mp)
                    stage[y, x] = st
                    break
                if st == 2:
                    out[y, x] = rgb[y // f, x // f]
                    if var is not None:
                        vout[y, x] = VCAP
                    stage[y, x] = 2
    return out, vout, stage


def _case(name, f, labels_lo, labels_hi, rgb_lo, albedo_lo=1.0, albedo_hi=1.0, var_lo=None, **kw):
    labels_lo, labels_hi = np.asarray(labels_lo, np.int32), np.asarray(labels_hi, np.int32)
    h, w = labels_lo.shape
    assert labels_hi.shape == (f * h, f * w)
    c = dict(name=name, f=f, labels_lo=labels_lo, labels_hi=labels_hi, rgb_lo=np.ascontiguousarray(rgb_lo, np.float32),
             g_lo=guides(labels_lo, f, albedo_lo), g_hi=guides(labels_hi, 1, albedo_hi), **kw)
    if var_lo is not None:
        c["var_lo"] = np.array(np.broadcast_to(np.asarray(var_lo, np.float32), (h, w, 3)))
    return c


def _const(h, w, rgb):
    return np.array(np.broadcast_to(np.asarray(rgb, np.float32), (h, w, 3)))


def cases():
    out = []
    # one plane, one colour, albedo 1: the interior weights sum to exactly 1 and the colour comes out unchanged (edges too: W·c / W)
    for f in (2, 4):
        out.append(_case(f"plane_const_f{f}", f, np.zeros((3, 4)), np.zeros((3 * f, 4 * f)), _const(3, 4, (0.5, 0.25, 0.75)),
                         closed="const", value=(0.5, 0.25, 0.75)))
    # a colour ramp linear in x: the exact bilinear values (clamped at the frame's edge, where the outside tap is skipped)
    for f in (2, 4):
        ramp = np.zeros((2, 5, 3), np.float32)
        ramp[:, :, 0], ramp[:, :, 1], ramp[:, :, 2] = np.arange(5) / 4.0, np.arange(5) / 2.0, np.arange(5)
        out.append(_case(f"ramp_x_f{f}", f, np.zeros((2, 5)), np.zeros((2 * f, 5 * f)), ramp, closed="ramp_x"))
    # all four corners and the edges: c = i + 4j; a corner sees one tap (W = b, out = that pixel), an edge two
    grid = np.zeros((3, 3, 3), np.float32)
    grid[:, :, 0] = np.arange(3)[None, :] + 4.0 * np.arange(3)[:, None]
    grid[:, :, 1], grid[:, :, 2] = grid[:, :, 0] / 8.0, 1.0
    out.append(_case("corners_f2", 2, np.zeros((3, 3)), np.zeros((6, 6)), grid, closed="corners"))
    # two perpendicular planes meeting along x = 4: no colour crosses the line
    lo = np.zeros((2, 4), np.int32)
    lo[:, 2:] = 1
    hi = np.zeros((4, 8), np.int32)
    hi[:, 4:] = 1
    col = _const(2, 4, (1.0, 0.0, 0.25))
    col[:, 2:] = (0.0, 1.0, 0.5)
    out.append(_case("two_planes_f2", 2, lo, hi, col, closed="two_planes"))
    # low-resolution albedo 1/2 under a full-size checker of 1/4 and 1: out = e·m_p with e = c / (1/2)
    chk = np.where(((np.arange(8)[None, :] + np.arange(6)[:, None]) & 1)[:, :, None] == 1, np.float32(0.25), np.float32(1.0))
    out.append(_case("albedo_checker_f2", 2, np.zeros((3, 4)), np.zeros((6, 8)), _const(3, 4, (0.5, 0.125, 0.75)), albedo_lo=0.5,
                     albedo_hi=np.broadcast_to(chk, (6, 8, 3)), closed="albedo", e=(1.0, 0.25, 1.5)))
    # f = 3 at a block centre: fx = fy = 0, one tap with b = 1 (checked at the block centres only: elsewhere thirds round)
    rgb3 = np.arange(27, dtype=np.float32).reshape(3, 3, 3) / 16.0
    centres = np.zeros((9, 9), bool)
    centres[1::3, 1::3] = True
    out.append(_case("f3_block_centre", 3, np.zeros((3, 3)), np.zeros((9, 9)), rgb3, check=centres, closed="f3"))
    # a background region beside a hit region: neither colour crosses (the sky's albedo is 0 and is never read)
    lo = np.zeros((2, 4), np.int32)
    lo[:, :2] = -1
    hi = np.zeros((4, 8), np.int32)
    hi[:, :4] = -1
    col = _const(2, 4, (0.25, 0.5, 0.125))
    col[:, :2] = (0.5, 0.75, 1.0)
    out.append(_case("background_f2", 2, lo, hi, col, albedo_lo=0.5, albedo_hi=0.5, closed="background"))
    # uniform variance v: var = v·Σb² / (Σb)²; 100/256·v in the interior at f = 2
    out.append(_case("uniform_var_f2", 2, np.zeros((3, 4)), np.zeros((6, 8)), _const(3, 4, (0.5, 0.25, 0.75)), var_lo=0.5, closed="var", v=0.5))
    # stage 1: the full column x = 8 lies in plane 1, which the low-resolution column 5 sees — outside that column's 2x2 footprint
    # (columns 3, 4) and inside its 4x4 (columns 2..5): the mean of column 5 over the footprint's rows, variance v / rows
    lo = np.zeros((4, 8), np.int32)
    lo[:, 5] = 1
    hi = np.zeros((8, 16), np.int32)
    hi[:, 8] = 1
    col = _const(4, 8, (0.5, 0.25, 0.75))
    col[:, 5] = (0.125, 1.0, 2.0)
    out.append(_case("stage1_strip_f2", 2, lo, hi, col, var_lo=0.25, closed="stage1"))
    # stage 2: the full pixel (5, 2) lies in plane 2, which no low-resolution pixel sees: the raw colour of low-resolution pixel
    # (2, 1) — not demodulated by its albedo 1/2, not modulated by the full pixel's 1/4 — and variance 2^32
    lo = np.zeros((3, 4), np.int32)
    hi = np.zeros((6, 8), np.int32)
    hi[2, 5] = 2
    col = np.arange(36, dtype=np.float32).reshape(3, 4, 3) / 32.0
    out.append(_case("stage2_pixel_f2", 2, lo, hi, col, albedo_lo=0.5, albedo_hi=0.25, var_lo=0.125, closed="stage2"))
    return out
