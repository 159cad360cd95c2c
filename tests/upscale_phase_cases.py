"""The CPU side of the tests of guided upscaling with a phase (DESIGN.md §4.20 "Lattice samples"; rayz_hip_upscaler_run_phase):
builds tests/upscale_phase_mirror.cpp and runs it on numpy arrays (`upscale`), and the hand cases with their answers in Fractions.

The cases are those of tests/upscale_cases.py in kind: LABEL maps of mutually perpendicular planes, between whose pixels the guide
weight is exactly 1 (same plane) or 0 (another), dyadic colours, albedos and variances, so that every product and sum of §4.20 is
exact and only the final divide rounds.  The low-resolution frame is a LATTICE of the full one: its guides are the full frame's at
(f·i + px, f·j + py) unless a case says otherwise.  `expected` works the answer out from the labels alone:

    sampled pixel whose own sample lies on its surface:   out = c_q,  var = clamp_var(var_q),  stage 0
    otherwise   out = (Σ b·e_q / Σ b)·m_p,   var = (Σ b²·ve_q / (Σ b)²)·m_p²   over the taps of the pixel's own surface,
    and with no such tap in the 4x4 footprint the raw colour of the nearest sample, clamp(floor((2a + f) / 2f), 0, w - 1) per axis."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile
from fractions import Fraction as Fr

import numpy as np

import upscale_cases
from upscale_ref import ALBEDO, Guides

HERE = os.path.dirname(os.path.abspath(__file__))
VCAP = np.float32(4294967296.0)

_lib = None
_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)


def load():
    global _lib
    if _lib is not None:
        return _lib
    gxx = shutil.which("g++")
    if not gxx:
        raise RuntimeError("no g++: the phase mirror cannot be built")
    so = os.path.join(tempfile.mkdtemp(prefix="upscale_phase_mirror_"), "upscale_phase_mirror.so")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "upscale_phase_mirror.cpp")],
                   check=True, capture_output=True, timeout=300)
    lib = C.CDLL(so)
    lib.upscale_phase_mirror.argtypes = [_F, _F, _I, _F, _F, _F, _I, _F, _F, _F, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_float, _F, _F, C.POINTER(C.c_uint8)]
    lib.upscale_phase_mirror.restype = None
    _lib = lib
    return lib


def upscale(rgb_lo, g_lo, g_hi, factor, phase, var_rgb=None, normal_power_log2=6, flags=ALBEDO, sigma_plane=0.25):
    """The run with a phase: (out, var or None, stage), shaped as tests/upscale_ref.py's `upscale` returns them."""
    lib = load()
    h, w = g_lo.index.shape
    H, W = g_hi.index.shape
    assert (H, W) == (factor * h, factor * w) and 0 <= phase[0] < factor and 0 <= phase[1] < factor
    rgb_lo = np.ascontiguousarray(rgb_lo, dtype=np.float32)
    assert rgb_lo.shape == (h, w, 3)
    if var_rgb is not None:
        var_rgb = np.ascontiguousarray(var_rgb, dtype=np.float32)
        assert var_rgb.shape == (h, w, 3)
    demod = bool(flags & ALBEDO)
    f = lambda a: a.ctypes.data_as(_F)  # noqa: E731
    i = lambda a: a.ctypes.data_as(_I)  # noqa: E731
    sp2 = np.float32(sigma_plane) * np.float32(sigma_plane)
    out = np.empty((H, W, 3), np.float32)
    var = np.empty((H, W, 3), np.float32) if var_rgb is not None else None
    stage = np.empty((H, W), np.uint8)
    lib.upscale_phase_mirror(f(rgb_lo), f(var_rgb) if var_rgb is not None else None, i(g_lo.index), f(g_lo.normal), f(g_lo.point),
                             f(g_lo.albedo) if demod else None, i(g_hi.index), f(g_hi.normal), f(g_hi.point), f(g_hi.albedo) if demod else None,
                             w, h, factor, phase[0], phase[1], normal_power_log2, float(sp2), f(out), f(var) if var is not None else None,
                             stage.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out, var, stage


def lattice(g, f, phase):
    """The guides of the lattice frame: the full frame's at (f·i + px, f·j + py), as `QueryResult.lattice` takes them."""
    px, py = phase
    return Guides(g.index[py::f, px::f], g.normal[py::f, px::f], g.point[py::f, px::f], None if g.albedo is None else g.albedo[py::f, px::f])


def _clamp_var(v):
    v = np.float32(v)
    return VCAP if not (v < VCAP) else (v if v > 0 else np.float32(0.0))


def expected(case):
    """(out, var or None, stage) of a case from its labels, in Fractions; pixels outside case['check'] are left 0."""
    f, (px, py) = case["f"], case["phase"]
    lab_lo, lab_hi = np.asarray(case["labels_lo"]), np.asarray(case["labels_hi"])
    h, w = lab_lo.shape
    H, W = lab_hi.shape
    rgb, var = case["rgb_lo"], case.get("var_lo")
    demod = case.get("flags", 1) & 1
    m_lo = case["g_lo"].albedo if demod else None
    m_hi = case["g_hi"].albedo if demod else None
    exact, round32 = upscale_cases._exact32, upscale_cases._round32

    def mod(alb, lab, j, i, c):
        if alb is None or lab[j, i] < 0:
            return Fr(1)
        return max(Fr(float(alb[j, i, c])), Fr(1, 256))

    def nearest(a, n):
        return min(max((2 * a + f) // (2 * f), 0), n - 1)  # (Python's // floors)

    out, vout, stage = np.zeros((H, W, 3), np.float32), (np.zeros((H, W, 3), np.float32) if var is not None else None), np.zeros((H, W), np.uint8)
    for y in range(H):
        for x in range(W):
            if "check" in case and not case["check"][y, x]:
                continue
            ax, ay = x - px, y - py
            i0, j0 = ax // f, ay // f
            rx, ry = ax - f * i0, ay - f * j0
            if rx == 0 and ry == 0 and lab_lo[j0, i0] == lab_hi[y, x]:  # its own sample, on its own surface (g = 1): passes through
                out[y, x] = rgb[j0, i0]
                if var is not None:
                    vout[y, x] = [_clamp_var(v) for v in var[j0, i0]]
                continue
            fx, fy = Fr(rx, f), Fr(ry, f)
            for st in (0, 1, 2):
                taps = []
                if st == 0:
                    taps = [(i0 + di, j0 + dj, (fx if di else 1 - fx) * (fy if dj else 1 - fy)) for dj in (0, 1) for di in (0, 1)]
                elif st == 1:
                    taps = [(i0 + di, j0 + dj, Fr(1)) for dj in (-1, 0, 1, 2) for di in (-1, 0, 1, 2)]
                taps = [(i, j, b) for i, j, b in taps if 0 <= i < w and 0 <= j < h and b != 0 and lab_lo[j, i] == lab_hi[y, x]]
                Wsum = sum(b for _, _, b in taps)
                if st < 2 and Wsum > 0:
                    exact(Wsum)
                    for c in range(3):
                        acc = sum(b * Fr(float(rgb[j, i, c])) / mod(m_lo, lab_lo, j, i, c) for i, j, b in taps)
                        exact(acc)
                        mp = mod(m_hi, lab_hi, y, x, c)
                        out[y, x, c] = exact(Fr(float(round32(acc / Wsum))) * mp)
                        if var is not None:
                            V = sum(b * b * Fr(float(var[j, i, c])) / mod(m_lo, lab_lo, j, i, c) ** 2 for i, j, b in taps)
                            exact(V), exact(Wsum * Wsum)
                            vout[y, x, c] = exact(Fr(float(round32(V / (Wsum * Wsum)))) * mp * mp)
                    stage[y, x] = st
                    break
                if st == 2:
                    out[y, x] = rgb[nearest(ay, h), nearest(ax, w)]
                    if var is not None:
                        vout[y, x] = VCAP
                    stage[y, x] = 2
    return out, vout, stage


def _case(name, f, phase, labels_hi, rgb_lo, albedo_hi=1.0, var_lo=None, labels_lo=None, **kw):
    labels_hi = np.asarray(labels_hi, np.int32)
    H, W = labels_hi.shape
    h, w = H // f, W // f
    g_hi = upscale_cases.guides(labels_hi, 1, albedo_hi)
    if labels_lo is None:  # a lattice of the full frame
        labels_lo, g_lo = labels_hi[phase[1]::f, phase[0]::f], lattice(g_hi, f, phase)
    else:                  # .. or a low-resolution frame that sees something else at its samples
        labels_lo = np.asarray(labels_lo, np.int32)
        g_lo = upscale_cases.guides(labels_lo, f, None if g_hi.albedo is None else 1.0)
    assert labels_lo.shape == (h, w)
    c = dict(name=name, f=f, phase=phase, labels_lo=labels_lo, labels_hi=labels_hi, rgb_lo=np.ascontiguousarray(rgb_lo, np.float32), g_lo=g_lo,
             g_hi=g_hi, **kw)
    if var_lo is not None:
        c["var_lo"] = np.array(np.broadcast_to(np.asarray(var_lo, np.float32), (h, w, 3)))
    return c


def ramp(x):
    """The full-frame colour ramp the ramp cases sample: linear in x, dyadic."""
    x = np.asarray(x, np.float64)
    return np.stack([x / 32.0, x / 4.0, x], axis=-1).astype(np.float32)


def cases():
    out = []
    const = lambda h, w, rgb: np.array(np.broadcast_to(np.asarray(rgb, np.float32), (h, w, 3)))  # noqa: E731
    for f, phase in ((2, (0, 0)), (2, (1, 1)), (4, (3, 0))):
        tag = f"f{f}_p{phase[0]}{phase[1]}"
        # one plane, one colour: the colour everywhere — W·c / W between the samples and at the edges, c itself at the samples
        out.append(_case(f"const_{tag}", f, phase, np.zeros((3 * f, 4 * f)), const(3, 4, (0.5, 0.25, 0.75)), closed="const", value=(0.5, 0.25, 0.75)))
        # a ramp linear in x, sampled at the lattice: between the first and the last sample the ramp ITSELF, full pixel by full pixel
        # (a lattice sample is a point of the frame); left of the first sample (i0 = -1) and right of the last (i0 + 1 = w) the
        # outside tap is skipped and the edge sample's value stays
        w = 5
        lo = np.broadcast_to(ramp(f * np.arange(w) + phase[0])[None], (2, w, 3))
        out.append(_case(f"ramp_x_{tag}", f, phase, np.zeros((2 * f, w * f)), lo, closed="ramp_x"))
    # both axes at once: c = x + 8y sampled at phase (1, 1); the top-left corner pixel (0, 0) has i0 = j0 = -1 and sees one tap
    x, y = np.meshgrid(np.arange(6), np.arange(6))
    full = np.stack([x + 8.0 * y, (x + 8.0 * y) / 8.0, np.ones_like(x, dtype=np.float64)], axis=-1).astype(np.float32)
    out.append(_case("corners_f2_p11", 2, (1, 1), np.zeros((6, 6)), full[1::2, 1::2], closed="corners", full=full))
    # a sampled pixel under DENOISE_ALBEDO with an albedo that is no power of two: the raw colour and the raw variance (clamped:
    # +inf -> 2^32, a negative one -> 0), not ((c / m) / 1)·m.  Checked at the sampled pixels only (elsewhere thirds round).
    rgb = (np.arange(36, dtype=np.float32).reshape(3, 4, 3) + 1) / 7.0
    var = np.full((3, 4, 3), 0.3, np.float32)
    var[0, 1], var[1, 2, 0], var[2, 3] = np.inf, -1.0, np.nan
    sampled = np.zeros((6, 8), bool)
    sampled[1::2, 0::2] = True
    out.append(_case("sampled_raw_f2_p01", 2, (0, 1), np.zeros((6, 8)), rgb, albedo_hi=(0.3, 0.7, 0.1), var_lo=var, check=sampled, closed="sampled"))
    # a sampled pixel whose sample lies on ANOTHER surface (the low-resolution G-buffer is not the lattice's here): no pass-through,
    # the pixel is rebuilt from the 4x4 footprint's taps of its own surface (stage 1: its 2x2 footprint is that one sample)
    lo = np.zeros((3, 4), np.int32)
    lo[1, 2] = 1
    col = const(3, 4, (0.5, 0.25, 0.75))
    col[1, 2] = (8.0, 8.0, 8.0)
    out.append(_case("sampled_refused_f2_p00", 2, (0, 0), np.zeros((6, 8)), col, labels_lo=lo, var_lo=0.25, closed="refused"))
    # stage 2: the full pixel (3, 1) lies on a surface no sample sees; at phase (0, 0) its nearest sample is (2, 1) — floor((2·3 +
    # 2) / 4), floor((2·1 + 2) / 4) — where the block rule x div f names (1, 0)
    hi = np.zeros((6, 8), np.int32)
    hi[1, 3] = 2
    col = np.arange(36, dtype=np.float32).reshape(3, 4, 3) / 32.0
    out.append(_case("stage2_nearest_f2_p00", 2, (0, 0), hi, col, albedo_hi=0.25, var_lo=0.125, closed="stage2"))
    return out
