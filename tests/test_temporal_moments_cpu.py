"""Temporal accumulation's moments mode without a GPU: the CPU restatement (tests/temporal_moments_mirror.cpp)
against the hand-derived exact answers of tests/temporal_moments_cases.py; its colour and length against the plain step's mirror,
bit for bit; a static sequence against numpy with exactly evaluated FMAs; two statistical conditions on the estimate; and the
binding — struct layout, prototypes, defaults, every RAYZ_ERR_BAD_ARG path of rayz_hip_temporal_step_moments (all checked before the
handle, so none needs a device), the ABI version."""
import ctypes as C
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest

import temporal_cases
import temporal_moments_cases as cases
import temporal_moments_ref as ref
import temporal_ref
from denoise_cases import round_f32
from rayz_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")
SIZES = [(1, 1), (5, 3), (33, 9), (45, 23)]
ORIGINS = [(0, 0), (0, 0), (0.25, -0.625), (1.25, 0.375)]  # first, static, a fractional move, a move by (1, 1) from there
VCAP = np.float32(2.0 ** 32)


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ; first at {bad[:5].tolist()}: " \
                          f"{[(got[tuple(b)], want[tuple(b)]) for b in bad[:3]]}"


def mirror_step(handle, s):
    return handle.step(s.rgb, s.index, s.normal, s.point, s.camera, s.spp, **s.params)


def frame_step(handle, f, spp=8, **params):
    return handle.step(f["rgb"], f["index"], f["normal"], f["point"], f["camera"], spp, **params)


def check_invariants(rgb, var, length, w2, index, what):
    """What §4.16 lists as following from its rules."""
    for a in (rgb, var, length, w2):
        assert np.isfinite(a).all(), what
    assert (w2 > 0).all() and (w2 <= 1).all(), what
    assert (var >= 0).all() and (var <= VCAP).all(), what
    assert (var[index < 0] == 0).all() and (w2[index < 0] == 1).all(), what


@pytest.mark.parametrize("case", cases.cases(), ids=lambda c: c.name)
def test_mirror_gives_the_hand_derived_answers(case):
    h, w = case.steps[0].index.shape
    m = ref.TemporalMoments(w, h)
    rgb, var, length, w2 = case.run(m, mirror_step)
    case.check(rgb, var, length, w2, "mirror")
    check_invariants(rgb, var, length, w2, case.steps[-1].index, case.name)
    c, v, g, p, mm = m.state()  # the history it left: the outputs, the guides, and {m2, W2}
    same_bits(c[..., :3], rgb, "history colour")
    same_bits(c[..., 3], length, "history length")
    same_bits(v[..., :3], var, "history variance")
    same_bits(mm[..., 3], w2, "history W2")
    assert (v[..., 3] == 0).all() and np.array_equal(g[..., 3].view(np.int32), case.steps[-1].index)
    if case.name == "one-pixel":  # m2 = c·c: (9/16, 9/64, 9/4)
        assert mm[0, 0].tolist() == [0.5625, 0.140625, 2.25, 1.0]
    if case.name == "static-two":  # m2 = (5, 5/4, 20)
        assert mm[0, 0].tolist() == [5.0, 1.25, 20.0, 0.5]


@pytest.mark.parametrize("w,h", SIZES)
def test_colour_and_length_are_the_plain_steps(w, h):
    """§4.16 step 1: for any sequence the colour and the length of a moments step equal the plain step's bit for bit — on the exact
    camera's sequence (first, static, a fractional move, a further move) and through the general camera, at the defaults and with
    alpha_min and n_max binding."""
    seqs = [("plane", temporal_cases.plane_sequence(w, h, 100 * w + h, ORIGINS)), ("general", temporal_cases.general_sequence(w, h, 5 * w + h))]
    for name, frames in seqs:
        for prm in ({}, dict(alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)):
            plain, mom = temporal_ref.Temporal(w, h), ref.TemporalMoments(w, h)
            for k, f in enumerate(frames):
                want = plain.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], 8, **prm)
                got = frame_step(mom, f, **prm)
                same_bits(got[0], want[0], f"{name} {w}x{h} step {k} colour")
                same_bits(got[2], want[2], f"{name} {w}x{h} step {k} length")
                check_invariants(*got, f["index"], f"{name} {w}x{h} step {k}")
                assert mom.last_static == plain.last_static
            hit = frames[-1]["index"] >= 0
            assert ((got[3] < 1) == (got[2] > 8))[hit].all()  # W2 < 1 exactly where history was found


def fma32(a, b, c):
    """fma(a, b, c) on float32 arrays, exactly: the rational a·b + c rounded once."""
    out = np.empty(a.shape, np.float32)
    for i in np.ndindex(a.shape):
        out[i] = round_f32(F(float(a[i])) * F(float(b[i])) + F(float(c[i])))
    return out


def clamp_var(v):
    with np.errstate(invalid="ignore"):
        return np.where(~(v < VCAP), VCAP, np.where(v > 0, v, np.float32(0))).astype(np.float32)


@pytest.mark.parametrize("w,h", SIZES)
def test_a_static_sequence_in_numpy(w, h):
    """alpha_min = 0, n_max = +inf, w2_max = 1 (the temporal estimate everywhere), one camera, 4 steps of 8 spp on synthetic guides:
    step k has al = f32(8 / 8k), kk = 1 - al, c = fma(al, c_k - c, c), m2 = fma(al, c_k·c_k - m2, m2), W2 = fma(kk·kk, W2, al·al) and
    v = clamp((max(m2 - c·c, 0)·W2) / (1 - W2)) on hits; c_k, c_k·c_k, 1 and 0 on background pixels — in numpy, the fma evaluated
    exactly.  On the first frame v = clamp(0/0) = 2^32 on hits."""
    frames = temporal_cases.plane_sequence(w, h, 17 * w + h, [(0, 0)] * 4)
    m = ref.TemporalMoments(w, h)
    hit = frames[0]["index"] >= 0
    hit3 = hit[..., None]
    c = m2 = W2 = None
    one = np.ones((h, w), np.float32)
    for k, f in enumerate(frames, 1):
        got = frame_step(m, f, alpha_min=0.0, n_max=INF, w2_max=1.0)
        x = f["rgb"]
        if k == 1:
            c, m2, W2 = x.copy(), x * x, one.copy()
        else:
            al = np.float32(8) / np.float32(8 * k)
            kk = np.float32(1) - al
            full = lambda a, like: np.full(like.shape, a, np.float32)  # noqa: E731
            cn = fma32(full(al, c), x - c, c)
            mn = fma32(full(al, c), x * x - m2, m2)
            wn = fma32(full(kk * kk, W2), W2, full(al * al, W2))
            c, m2, W2 = np.where(hit3, cn, x), np.where(hit3, mn, x * x), np.where(hit, wn, one)
        e = m2 - c * c
        with np.errstate(invalid="ignore", divide="ignore"):
            v = clamp_var((np.where(e > 0, e, np.float32(0)) * W2[..., None]) / (np.float32(1) - W2[..., None]))
        v = np.where(hit3, v, np.float32(0)).astype(np.float32)
        same_bits(got[0], c, f"{w}x{h} step {k} colour")
        same_bits(got[1], v, f"{w}x{h} step {k} variance")
        same_bits(got[2], np.where(hit, np.float32(8 * k), np.float32(8)).astype(np.float32), f"{w}x{h} step {k} length")
        same_bits(got[3], W2.astype(np.float32), f"{w}x{h} step {k} W2")
        same_bits(m.state()[4][..., :3], m2.astype(np.float32), f"{w}x{h} step {k} m2")
        if k == 1:
            assert (got[1][hit] == VCAP).all()
        else:
            assert abs(float(W2[hit].max()) - 1 / k) < 1e-6 if hit.any() else True


def noisy_flat_frames(seed, count, w=45, h=23, sigma=0.1):
    """Constant colour 0.5 plus N(0, sigma²) per channel, fresh per frame, on flat guides: one hittable, one normal, the exact camera."""
    rng = np.random.default_rng(seed)
    s = cases.MStep(w, h, cases.cam(), 0)
    for _ in range(count):
        rgb = (0.5 + sigma * rng.standard_normal((h, w, 3))).astype(np.float32)
        yield dict(rgb=rgb, index=s.index, normal=s.normal, point=s.point, camera=s.camera)


@pytest.mark.parametrize("seed", range(5))
def test_first_frame_estimate_is_unbiased(seed):
    """The spatial estimate of a first frame: mean(v_out) / sigma² within [0.95, 1.05] (a float32 numpy simulation of the contract
    gave 0.982 .. 1.013 over these seeds; the mirror gives 0.9825 .. 1.0130)."""
    (f,) = noisy_flat_frames(seed, 1)
    _, var, _, w2 = frame_step(ref.TemporalMoments(45, 23), f, spp=1)
    ratio = float(var.astype(np.float64).mean()) / 0.01
    print(f"seed {seed}: first frame mean(v) / sigma^2 = {ratio:.4f}")
    assert (w2 == 1).all() and 0.95 <= ratio <= 1.05, ratio


@pytest.mark.parametrize("alpha_min", [0.0, 0.05])
@pytest.mark.parametrize("seed", range(5))
def test_temporal_estimate_after_32_static_frames_is_unbiased(seed, alpha_min):
    """After 32 static frames: mean(v_out) / (sigma²·mean(W2)) within [0.95, 1.05], for the running mean (alpha_min = 0) and for the
    exponential average alpha_min = 0.05 settles into (the simulation gave 0.986 .. 1.008; the mirror gives 0.9945 .. 1.0021)."""
    m = ref.TemporalMoments(45, 23)
    for f in noisy_flat_frames(seed, 32):
        _, var, length, w2 = frame_step(m, f, spp=1, alpha_min=alpha_min)
    assert (w2 < 0.25).all() and (length == 32).all()  # the temporal estimate everywhere
    if alpha_min == 0.0:
        assert abs(float(w2.mean()) - 1 / 32) < 1e-6
    ratio = float(var.astype(np.float64).mean()) / (0.01 * float(w2.astype(np.float64).mean()))
    print(f"seed {seed}, alpha_min {alpha_min}: after 32 frames mean(v) / (sigma^2 mean(W2)) = {ratio:.4f}")
    assert 0.95 <= ratio <= 1.05, ratio


# ---- the binding --------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayz_hip.h")).read(), flags=re.S)


def test_struct_layout_and_defaults_match_the_header(built):
    hdr = _header()
    m = re.search(r"typedef struct RayzTemporalMomentsParams \{(.*?)\} RayzTemporalMomentsParams;", hdr, flags=re.S)
    decls = [d.split() for d in m.group(1).split(";") if d.split()]
    assert all(d[0] == "double" for d in decls)
    assert [d[1] for d in decls] == ["w2_max", "min_taps"] == [n for n, _ in capi.TemporalMomentsParams._fields_]
    assert all(t is C.c_double for _, t in capi.TemporalMomentsParams._fields_) and C.sizeof(capi.TemporalMomentsParams) == 16
    assert set(capi.TEMPORAL_MOMENTS_DEFAULTS) == {"w2_max", "min_taps"} and not set(capi.TEMPORAL_MOMENTS_DEFAULTS) & set(capi.TEMPORAL_DEFAULTS)
    for k, v in capi.TEMPORAL_MOMENTS_DEFAULTS.items():
        assert float(re.search(rf"RAYZ_TEMPORAL_MOMENTS_DEFAULT_{k.upper()} (\S+)", hdr).group(1)) == v == ref.MOMENTS_DEFAULTS[k]
    assert len(re.findall(r"RAYZ_TEMPORAL_DEFAULT_\w+ ", hdr)) == 4  # the plain step's four, untouched
    assert capi.TEMPORAL_DEFAULTS == temporal_ref.DEFAULTS


def test_prototypes_in_header_and_binding(built):
    hdr = " ".join(_header().split())
    assert "int rayz_hip_temporal_track_moments(RayzTemporal* tm);" in hdr
    assert ("int rayz_hip_temporal_step_moments(RayzTemporal* tm, const RayzTemporalParams* params_or_null, "
            "const RayzTemporalMomentsParams* mparams_or_null, const RayzCameraDesc* camera, uint32_t spp, const float* d_rgb_in, "
            "const RayzQueryOutputs* gbuffer, float* d_rgb_out, float* d_var_out, float* d_length_out_or_null, float* d_w2_out_or_null, "
            "void* hip_stream);") in hdr
    protos = {p[0]: p for p in capi.PROTOTYPES}
    assert [len(protos["rayz_hip_temporal_" + k][2]) for k in ("track_moments", "step_moments", "step")] == [1, 12, 11]
    lib = capi.load()
    assert hasattr(lib, "rayz_hip_temporal_track_moments") and hasattr(lib, "rayz_hip_temporal_step_moments")
    assert lib.rayz_hip_abi_version() == capi.ABI_VERSION == 5


def test_every_bad_argument_is_refused_before_the_handle(built):
    """All arguments are checked before the handle and nothing touches a device: with valid arguments and a null handle the answer is
    RAYZ_ERR_STATE, with any one bad argument RAYZ_ERR_BAD_ARG and a message that names it."""
    lib = capi.load()
    buf, other = C.c_void_p(4096), C.c_void_p(8192)  # never dereferenced: the handle is refused first
    g = capi.QueryOutputs(index=4096, normal=4096, point=4096)
    good = capi.CameraDesc(look_from=(0, 0, -8), px_du=(1, 0, 0), px_dv=(0, 1, 0), px_origin=(0, 0, 0))

    def run(prm=None, mprm=None, cam=good, spp=8, rgb=buf, gb=g, out=other, vout=buf, length=None, w2=None, **over):
        tp = {k: v for k, v in over.items() if k in capi.TEMPORAL_DEFAULTS}
        mp = {k: v for k, v in over.items() if k in capi.TEMPORAL_MOMENTS_DEFAULTS}
        assert len(tp) + len(mp) == len(over)
        p = capi.TemporalParams(**{**capi.TEMPORAL_DEFAULTS, **tp}) if prm is None else prm
        q = capi.TemporalMomentsParams(**{**capi.TEMPORAL_MOMENTS_DEFAULTS, **mp}) if mprm is None else mprm
        return lib.rayz_hip_temporal_step_moments(None, C.byref(p) if p is not False else None, C.byref(q) if q is not False else None,
                                                  C.byref(cam) if cam is not None else None, spp, rgb, C.byref(gb) if gb is not None else None,
                                                  out, vout, length, w2, None)

    assert run() == capi.ERR_STATE and b"not a temporal handle" in lib.rayz_hip_last_error()
    assert run(prm=False) == capi.ERR_STATE and run(mprm=False) == capi.ERR_STATE and run(prm=False, mprm=False) == capi.ERR_STATE
    assert run(length=buf) == capi.ERR_STATE and run(w2=buf) == capi.ERR_STATE and run(length=buf, w2=buf) == capi.ERR_STATE
    assert run(spp=1) == capi.ERR_STATE and run(spp=1 << 24) == capi.ERR_STATE
    assert run(alpha_min=0.0, n_max=INF, normal_cos_min=-1.0, max_rel_dist=INF, w2_max=0.0, min_taps=2.0) == capi.ERR_STATE
    assert run(alpha_min=1.0, n_max=1.0, normal_cos_min=1.0, max_rel_dist=1e-30, w2_max=1.0, min_taps=49.0) == capi.ERR_STATE
    bad = [(dict(alpha_min=-0.01), b"alpha_min"), (dict(alpha_min=1.01), b"alpha_min"), (dict(alpha_min=NAN), b"alpha_min"),
           (dict(n_max=0.5), b"n_max"), (dict(n_max=NAN), b"n_max"), (dict(n_max=-INF), b"n_max"),
           (dict(normal_cos_min=-1.5), b"normal_cos_min"), (dict(normal_cos_min=1.5), b"normal_cos_min"), (dict(normal_cos_min=NAN), b"normal_cos_min"),
           (dict(max_rel_dist=0.0), b"max_rel_dist"), (dict(max_rel_dist=-1.0), b"max_rel_dist"), (dict(max_rel_dist=NAN), b"max_rel_dist"),
           (dict(spp=0), b"spp"), (dict(spp=(1 << 24) + 1), b"spp"),
           (dict(w2_max=-0.01), b"w2_max"), (dict(w2_max=1.01), b"w2_max"), (dict(w2_max=NAN), b"w2_max"), (dict(w2_max=INF), b"w2_max"),
           (dict(min_taps=1.99), b"min_taps"), (dict(min_taps=49.01), b"min_taps"), (dict(min_taps=NAN), b"min_taps"),
           (dict(min_taps=0.0), b"min_taps"), (dict(min_taps=INF), b"min_taps")]
    for over, word in bad:
        assert run(**over) == capi.ERR_BAD_ARG, over
        assert word in lib.rayz_hip_last_error(), (over, lib.rayz_hip_last_error())
    for missing in ("rgb", "out", "vout", "gb", "cam"):
        assert run(**{missing: None}) == capi.ERR_BAD_ARG, missing
    assert run(vout=None) == capi.ERR_BAD_ARG and b"variance" in lib.rayz_hip_last_error()
    assert run(out=buf) == capi.ERR_BAD_ARG and b"in place" in lib.rayz_hip_last_error()  # d_rgb_out == d_rgb_in
    for field in ("index", "normal", "point"):
        part = capi.QueryOutputs(**{k: 4096 for k in ("index", "normal", "point", "albedo") if k != field})
        assert run(gb=part) == capi.ERR_BAD_ARG and b"index, normal and point" in lib.rayz_hip_last_error()
    cams = [capi.CameraDesc(look_from=(0, 0, -8), px_du=(1, 0, 0), px_dv=(2, 0, 0), px_origin=(0, 0, 0)),
            capi.CameraDesc(look_from=(0, 0, 0), px_du=(1, 0, 0), px_dv=(0, 1, 0), px_origin=(3, 4, 0)),
            capi.CameraDesc(look_from=(0, 0, NAN), px_du=(1, 0, 0), px_dv=(0, 1, 0), px_origin=(0, 0, 0)),
            capi.CameraDesc()]
    for cam in cams:
        assert run(cam=cam) == capi.ERR_BAD_ARG and b"det" in lib.rayz_hip_last_error()
    assert lib.rayz_hip_temporal_track_moments(None) == capi.ERR_STATE and b"not a temporal handle" in lib.rayz_hip_last_error()
