"""Known answers worked out by hand from the reference's text, for the functions its own tests leave unpinned.

Every other parity check compares this repository's code with this repository's code (device == mode B bit for bit,
mode B ~ mode A, all three == tests/golden/kat_frozen.npz).  A line of the Zig misread the same way in mode A and
mode B would pass all of them.  The records of tests/golden/hand_vectors.json were derived from the Zig text in
closed form — each carries the reference line and the derivation in its `why` — and hold:

* `hitInner` + `Hit.init` (SPHERE_HIT), `reflectance`, every `scatter` with `reflect` / `refract` (SCATTER), the
  checker parity, the background and `getRay`'s draw order, through mode A, mode B (f32, f64) and, with `-m gpu`,
  the HIP device functions (`rayz_hip_kat`) in both precisions;
* `bounceRay`'s depth, background and attenuation product (which no KAT op returns) through closed-form renders of
  nearly-one-ray frames (vfov 0.001°) in mode A, mode B and on the GPU through the flat list and the BVH.

Decisions (hit, front_face, scattered, draw count, checker parity) must be exact; values are held within 1e-12 in
f64 and 1e-6 in f32 (relative above 1).  Inputs and uniforms are dyadic, so f32 and f64 start from the same numbers.
"""
import json
import math
import os
import re

import numpy as np
import pytest

from rayz_amd import capi, tracer

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hand_vectors.json")
with open(PATH) as _f:
    VECTORS = json.load(_f)
NAMES = [v["name"] for v in VECTORS]

OPS = {"REFRACT": capi.KAT_REFRACT, "REFLECTANCE": capi.KAT_REFLECTANCE, "GET_RAY": capi.KAT_GET_RAY,
       "SPHERE_HIT": capi.KAT_SPHERE_HIT, "SCATTER": capi.KAT_SCATTER, "CHECKER": capi.KAT_CHECKER,
       "BACKGROUND": capi.KAT_BACKGROUND}
# field -> slot in the record (include/rayz_hip.h: RayzKatOp); the uniform count and list follow at N_U, N_U + 1
IN = {
    "REFRACT": {"unit_dir": 0, "normal": 3, "eta": 6},
    "REFLECTANCE": {"cos": 0, "ri": 1},
    "GET_RAY": {"look_from": 0, "px_du": 3, "px_dv": 6, "px_origin": 9, "defocus_u": 12, "defocus_v": 15,
                "defocus": 18, "px": 19, "py": 20, "n_u": 21},
    "SPHERE_HIT": {"center": 0, "velocity": 3, "radius": 6, "origin": 7, "dir": 10, "time": 13, "tmin": 14, "tmax": 15},
    "SCATTER": {"kind": 0, "method": 1, "param": 2, "ray_origin": 3, "dir": 6, "point": 9, "normal": 12,
                "front_face": 15, "n_u": 16},
    "CHECKER": {"point": 0, "scale": 3},
    "BACKGROUND": {"dir": 0},
}
OUT = {
    "REFRACT": {"dir": 0},
    "REFLECTANCE": {"r": 0},
    "GET_RAY": {"origin": 0, "dir": 3, "time": 6, "draws": 7},
    "SPHERE_HIT": {"hit": 0, "t": 1, "point": 2, "normal": 5, "front_face": 8},
    "SCATTER": {"scattered": 0, "dir": 1, "draws": 4},
    "CHECKER": {"parity": 0},
    "BACKGROUND": {"colour": 0},
}
DECISIONS = {"hit", "front_face", "scattered", "draws", "parity"}
TOL = {"a": 1e-12, F64: 1e-12, F32: 1e-6}


def _num(x):
    return math.inf if x == "inf" else float(x)


def pack(v):
    """One record of `v` in the RAYZ_KAT_IN_STRIDE layout."""
    rec = np.zeros(capi.KAT_IN_STRIDE)
    slots = IN[v["op"]]
    for k, x in v["in"].items():
        at = slots[k]
        vals = [_num(y) for y in x] if isinstance(x, list) else [_num(x)]
        rec[at:at + len(vals)] = vals
    if "u" in v:
        n_at = slots["n_u"]
        rec[n_at] = len(v["u"])
        rec[n_at + 1:n_at + 1 + len(v["u"])] = v["u"]
    return rec


def check(v, out, tol, what):
    """`out`: one KAT_OUT_STRIDE row.  Decisions exactly, values within tol (relative above magnitude 1)."""
    slots = OUT[v["op"]]
    for k, want in v["want"].items():
        want = np.atleast_1d(np.array(want, dtype=np.float64))
        got = out[slots[k]:slots[k] + len(want)]
        if k in DECISIONS:
            assert got.tolist() == want.tolist(), f"{what} {v['name']}: {k} = {got.tolist()}, hand-derived {want.tolist()}"
        else:
            bound = tol * np.maximum(1.0, np.abs(want))
            assert (np.abs(got - want) <= bound).all(), \
                f"{what} {v['name']}: {k} = {got.tolist()}, hand-derived {want.tolist()} (tolerance {tol})"
    if v["op"] == "SPHERE_HIT" and v["want"]["hit"] == 1:
        assert out[9] == 1, f"{what} {v['name']}: a hit the reject test did not pass on"


def by_name(name):
    return next(v for v in VECTORS if v["name"] == name)


# ---- the file itself ----------------------------------------------------------------------------------------------
def test_hand_vector_file_is_well_formed():
    assert len(VECTORS) >= 45 and len(set(NAMES)) == len(NAMES)
    cite = re.compile(r"src/\w+\.zig:\d+")
    for v in VECTORS:
        assert v["op"] in OPS and cite.search(v["why"]), v["name"]
        assert set(v["in"]) <= set(IN[v["op"]]) and set(v["want"]) <= set(OUT[v["op"]]), v["name"]
        rec = pack(v)
        fin = rec[np.isfinite(rec)]
        assert np.array_equal(fin.astype(np.float32).astype(np.float64), fin), f"{v['name']}: input not exact in f32"
        u = np.array(v.get("u", []), dtype=np.float64)
        assert ((u >= 0) & (u < 1) & (u * 2.0 ** 24 == np.floor(u * 2.0 ** 24))).all(), f"{v['name']}: u not k/2^24"
    ops = {v["op"] for v in VECTORS}
    assert ops == set(OPS), set(OPS) - ops


# ---- CPU: oracle mode A (the reference as written) and mode B (kernel arithmetic) ---------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_mode_a_matches_hand_vector(oracle, name):
    v = by_name(name)
    out = oracle.kat_a(OPS[v["op"]], pack(v)[None])[0]
    check(v, out, TOL["a"], "mode A")


@pytest.mark.parametrize("prec", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("name", NAMES)
def test_mode_b_matches_hand_vector(oracle, name, prec):
    v = by_name(name)
    out = oracle.kat_b(OPS[v["op"]], pack(v)[None], prec)[0]
    check(v, out, TOL[prec], f"mode B {'f32' if prec == F32 else 'f64'}")


# ---- GPU: the trace kernels' own device functions ------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prec", [F32, F64], ids=["f32", "f64"])
def test_device_functions_match_hand_vectors(gpu, oracle, prec):
    """All records, one rayz_hip_kat launch per op: the hand-derived answers, and mode B bit for bit."""
    for opname, op in OPS.items():
        vs = [v for v in VECTORS if v["op"] == opname]
        rec = np.stack([pack(v) for v in vs])
        got, want_b = gpu.kat(op, rec, prec), oracle.kat_b(op, rec, prec)
        for i, v in enumerate(vs):
            check(v, got[i], TOL[prec], f"device {'f32' if prec == F32 else 'f64'}")
        same = (got == want_b) | (np.isnan(got) & np.isnan(want_b))
        assert same.all(), (opname, [vs[i]["name"] for i in np.flatnonzero(~same.all(1))])


# ---- closed-form renders: bounceRay's depth, background and attenuation product -----------------------------------
# Frames of W x H pixels at vfov 0.001°: every primary ray is within THETA of the view axis (half the viewport diagonal).
W, VFOV = 32, 0.001
THETA = math.atan(math.tan(math.radians(VFOV) / 2) * math.hypot(1.0, 16.0 / 9.0))
SKY_UP = np.array([0.5, 0.7, 1.0])
T45 = (1 + 1 / math.sqrt(2)) / 2  # background((0,1,1)/sqrt2): t = (1 + 1/sqrt2)/2, ((1 - t) + c) t
SKY_45 = ((1 - T45) + SKY_UP) * T45  # (0.5517766953, 0.7224873734, 0.9785533906)
# A direction within angle e of a closed-form one moves unit(d).y by at most e, and each background channel
# ((1 - t) + c) t, t = (y + 1)/2, by at most |d/dy| <= 1 times that; mirrors tilt by at most the ray's own e (plus
# e·|o - p|/R from the floor sphere's curvature, R = 100).  3·THETA (5.3e-5) covers both; 1e-6 is f32 rounding.
SPREAD_TOL = 3 * THETA + 1e-6
A_COLOUR = np.array([0.75, 0.5, 0.25])


def _tracer(look_from, look_at, vup=(0, 1, 0), spp=4, bounces=2, w=W):
    dist = float(np.linalg.norm(np.subtract(look_at, look_from)))
    t = tracer.Tracer.init(w, VFOV, dist, 0.0, look_from, look_at, vup, seed=5)
    t.samples_per_px, t.max_bounces = spp, bounces
    t.set_gpu(render_seed=7)
    return t


def _cpu_renders(oracle, t):
    """(label, image) for mode A (f64, the reference's tmin 1e-10, its own stream) and mode B in f32 and f64."""
    sd, cam = t.scene_desc(), t.camera_desc()
    pa = t.params()
    pa.precision, pa.tmin = F64, 1e-10
    img, _ = oracle.render_a(sd, cam, pa, t.rng_state().copy())
    yield "mode A", img
    for prec in (F32, F64):
        t.set_gpu(precision=prec)
        img, _ = oracle.render_b(sd, cam, t.params())
        yield f"mode B {'f32' if prec == F32 else 'f64'}", img.astype(np.float64)
    t.set_gpu(precision=F32)


def _gpu_renders(gpu, oracle, t):
    """(label, image) on the GPU, f32 and f64, through the flat list and the BVH; each equal to mode B bit for bit."""
    sd, cam = t.scene_desc(), t.camera_desc()
    for prec in (F32, F64):
        t.set_gpu(precision=prec)
        want_b, _ = oracle.render_b(sd, cam, t.params())
        for trav in (capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH):
            p = t.params()
            p.traversal = trav
            img, _ = gpu.render_host(sd, cam, p)
            label = f"GPU {'f32' if prec == F32 else 'f64'} {'flat list' if trav == capi.TRAVERSAL_LINEAR else 'BVH'}"
            assert np.array_equal(img, want_b), f"{label}: differs from mode B"
            yield label, img.astype(np.float64)
    t.set_gpu(precision=F32)


def _nested_checker_pool(pool):
    """even/odd at scale 1, each a checker again: even -> scale 0.25 (A, B), odd -> scale 0.5 (C, D)."""
    a, b = pool.add_solid_texture(LEAF["A"]), pool.add_solid_texture(LEAF["B"])
    c, d = pool.add_solid_texture(LEAF["C"]), pool.add_solid_texture(LEAF["D"])
    return pool.add_checker_texture(1.0, pool.add_checker_texture(0.25, a, b), pool.add_checker_texture(0.5, c, d))


LEAF = {"A": (0.75, 0.5, 0.25), "B": (0.25, 0.75, 0.5), "C": (0.5, 0.25, 0.75), "D": (1.0, 0.5, 0.125)}
# Aim points on the mirror's top (y = 0.3, every coordinate >= 0.05 inside its cell at both levels; the hit points lie
# within 1e-4 of the aim).  Outer parity mod(floor(x) + floor(y) + floor(z), 2) at scale 1, then the inner checker's:
CHECKER_AIMS = {
    "A": (0.3, 0.3, 0.6),     # outer 0+0+0 = 0 even; inner (scale 0.25) 1+1+2 = 4 even -> A
    "B": (-2.6, 0.3, -0.7),   # outer -3+0-1 = -4 even; inner -11+1-3 = -13, mod 1 odd -> B
    "C": (-0.7, 0.3, 0.2),    # outer -1+0+0 = -1, mod 1 odd; inner (scale 0.5) -2+0+0 = -2, mod 0 even -> C
    "D": (1.7, 0.3, 0.45),    # outer 1+0+0 = 1 odd; inner (scale 0.5) 3+0+0 = 3 odd -> D
}


def _scene(kind, bounces=2, aim=None):
    """The closed-form scenes.  Returns (tracer, expected pixel (3,), tolerance)."""
    if kind == "inside_closed_sphere":  # the camera inside a closed diffuse sphere, itself inside a second one
        t = _tracer((0, 0, 0), (0, 0, 1), bounces=bounces)
        m = t.pool.add_diffuse(t.pool.add_solid_texture((0.9, 0.9, 0.9)))
        t.pool.add_sphere((0, 0, 0), 10.0, m)
        t.pool.add_sphere((0, 0, 0), 20.0, m)
        return t, np.zeros(3), 0.0
    if kind == "sphere_fills_footprint":  # a diffuse sphere ahead covers every primary ray's path
        t = _tracer((0, 0, -5), (0, 0, 0), bounces=bounces)
        t.pool.add_sphere((0, 0, 0), 1.0, t.pool.add_diffuse(t.pool.add_solid_texture((0.9, 0.9, 0.9))))
        return t, np.zeros(3), 0.0
    if kind in ("sky_up", "sky_x", "sky_down"):  # empty pool: every primary ray misses
        at = {"sky_up": (0, 1, 0), "sky_x": (1, 0, 0), "sky_down": (0, -1, 0)}[kind]
        t = _tracer((0, 0, 0), at, vup=(0, 0, 1) if kind != "sky_x" else (0, 1, 0), bounces=bounces)
        want = {"sky_up": SKY_UP, "sky_x": np.array([0.5, 0.6, 0.75]), "sky_down": np.zeros(3)}[kind]
        return t, (want if bounces >= 1 else np.zeros(3)), SPREAD_TOL
    if kind == "mirror":  # a fuzz-0 metal floor sphere (top at the origin) seen 45° down from (0,1,-1)
        t = _tracer((0, 1, -1), (0, 0, 0), bounces=bounces)
        t.pool.add_sphere((0, -100, 0), 100.0, t.pool.add_metallic(t.pool.add_solid_texture(A_COLOUR), 0.0))
        return t, (A_COLOUR * SKY_45 if bounces >= 2 else np.zeros(3)), SPREAD_TOL
    if kind == "nested_checker":
        p = np.array(CHECKER_AIMS[aim])
        t = _tracer(tuple(p + [0, 1, -1]), tuple(p), bounces=bounces)
        tex = _nested_checker_pool(t.pool)
        t.pool.add_sphere(tuple(p - [0, 100, 0]), 100.0, t.pool.add_metallic(tex, 0.0))
        return t, np.array(LEAF[aim]) * SKY_45, SPREAD_TOL
    raise ValueError(kind)


CLOSED_FORM = [("inside_closed_sphere", 0, None), ("inside_closed_sphere", 1, None), ("inside_closed_sphere", 2, None),
               ("sphere_fills_footprint", 0, None), ("sphere_fills_footprint", 1, None),
               ("sky_up", 1, None), ("sky_up", 0, None), ("sky_x", 1, None), ("sky_down", 1, None),
               ("mirror", 2, None), ("mirror", 3, None), ("mirror", 1, None)] + \
              [("nested_checker", 2, k) for k in CHECKER_AIMS]
CLOSED_IDS = [f"{k}-b{b}" + (f"-{a}" if a else "") for k, b, a in CLOSED_FORM]


def _hold(label, img, want, tol, what):
    err = np.abs(img - want).max()
    assert err <= tol, f"{what}, {label}: max |pixel - closed form {want.tolist()}| = {err:.3e} > {tol:.1e}"


@pytest.mark.parametrize("kind,bounces,aim", CLOSED_FORM, ids=CLOSED_IDS)
def test_closed_form_render_cpu(oracle, kind, bounces, aim):
    t, want, tol = _scene(kind, bounces, aim)
    for label, img in _cpu_renders(oracle, t):
        _hold(label, img, want, tol, CLOSED_IDS[CLOSED_FORM.index((kind, bounces, aim))])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,bounces,aim", CLOSED_FORM, ids=CLOSED_IDS)
def test_closed_form_render_gpu(gpu, oracle, kind, bounces, aim):
    t, want, tol = _scene(kind, bounces, aim)
    for label, img in _gpu_renders(gpu, oracle, t):
        _hold(label, img, want, tol, CLOSED_IDS[CLOSED_FORM.index((kind, bounces, aim))])


# Glass: the camera looks straight up through an ior-1.5 unit sphere.  At normal incidence every interface reflects
# with r0 = ((1 - 1.5)/(1 + 1.5))^2 = 0.04 whichever side the ray is on (src/material.zig:179-183 with cos = 1); light
# leaves upward after 2k + 2 interfaces with probability (1 - r0)^2 r0^(2k), so in total (1 - r0)^2 / (1 - r0^2) =
# (1 - r0)/(1 + r0) = 0.923077, times the upward background (0.5,0.7,1.0); downward light meets a background of
# exactly 0.  20 bounces leave r0^18 ~ 1e-25 of the series out.  Each sample is 0 or the full colour (Bernoulli).
GLASS_P = (1 - 0.04) / (1 + 0.04)
GLASS_W, GLASS_SPP = 64, 512  # 64 x 36 x 512 = 1,179,648 samples


def _glass():
    t = _tracer((0, -10, 0), (0, 0, 0), vup=(0, 0, 1), spp=GLASS_SPP, bounces=20, w=GLASS_W)
    t.pool.add_sphere((0, 0, 0), 1.0, t.pool.add_dielectric(1.5))
    return t


def _hold_glass(label, img):
    n = img.shape[0] * img.shape[1] * GLASS_SPP
    frac = img.reshape(-1, 3) / SKY_UP  # each pixel: the fraction of its samples that left upward
    assert np.abs(frac - frac[:, :1]).max() < 1e-5, f"{label}: channels are not one fraction of (0.5,0.7,1.0)"
    p = frac.mean()
    se = math.sqrt(GLASS_P * (1 - GLASS_P) / n)
    assert abs(p - GLASS_P) < 5 * se, f"{label}: {p:.6f} vs (1 - r0)/(1 + r0) = {GLASS_P:.6f}, {(p - GLASS_P) / se:+.2f} SE"


def test_glass_render_cpu(oracle):
    for label, img in _cpu_renders(oracle, _glass()):
        _hold_glass(label, img)


@pytest.mark.gpu
def test_glass_render_gpu(gpu, oracle):
    for label, img in _gpu_renders(gpu, oracle, _glass()):
        _hold_glass(label, img)
