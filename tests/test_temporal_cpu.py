"""Temporal accumulation without a GPU: the CPU restatement (tests/temporal_mirror.cpp) against the hand-derived
exact answers of tests/temporal_cases.py; a static sequence against the running mean and an integer shift against numpy slicing,
both evaluated with the same f32 operations; and the binding — struct layout, prototypes, defaults, every RAYZ_ERR_BAD_ARG path
of rayz_hip_temporal_step (all checked before the handle, so none needs a device), the ABI version."""
import ctypes as C
import os
import re
from fractions import Fraction as F

import numpy as np
import pytest

import temporal_cases as cases
import temporal_ref
from denoise_cases import round_f32
from rayz_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")
NAN = float("nan")
SIZES = [(1, 1), (5, 3), (33, 9), (45, 23)]


def mirror_step(handle, s):
    return handle.step(s.rgb, s.var, s.index, s.normal, s.point, s.camera, s.spp, **s.params)


def frame_step(handle, f, spp=8, **params):
    return handle.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], spp, **params)


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ; first at {bad[:5].tolist()}: " \
                          f"{[(got[tuple(b)], want[tuple(b)]) for b in bad[:3]]}"


@pytest.mark.parametrize("case", cases.cases(), ids=lambda c: c.name)
def test_mirror_gives_the_hand_derived_answers(case):
    h, w = case.steps[0].index.shape
    rgb, var, length = case.run(temporal_ref.Temporal(w, h), mirror_step)
    case.check(rgb, var, length, "mirror")
    assert np.isfinite(rgb).all() and np.isfinite(var).all() and np.isfinite(length).all() and (var >= 0).all()


def test_the_exact_camera_has_the_matrix_the_cases_derive():
    """M = [[1, 0, -ox/8], [0, 1, -oy/8], [0, 0, 1/8]] and from = (0, 0, -8); a camera that spans no volume, or holds a NaN or an
    infinity, has none."""
    M, fr = temporal_ref.camera_matrix(cases.cam(F(-1, 2), 3))
    assert M.tolist() == [1, 0, 0.0625, 0, 1, -0.375, 0, 0, 0.125] and fr.tolist() == [0, 0, -8]
    flat = dict(cases.cam(), px_dv=(2.0, 0.0, 0.0))  # px_dv parallel to px_du
    assert temporal_ref.camera_matrix(flat) is None
    assert temporal_ref.camera_matrix(dict(cases.cam(), look_from=(0.0, 0.0, 0.0))) is None  # the lens centre in the pixel plane
    assert temporal_ref.camera_matrix(dict(cases.cam(), px_origin=(NAN, 0.0, 0.0))) is None
    assert temporal_ref.camera_matrix(dict(cases.cam(), px_du=(INF, 0.0, 0.0))) is None


def fma32(a, b, c):
    """fma(a, b, c) on float32 arrays, exactly: the rational a·b + c rounded once."""
    out = np.empty(a.shape, np.float32)
    for i in np.ndindex(a.shape):
        out[i] = round_f32(F(float(a[i])) * F(float(b[i])) + F(float(c[i])))
    return out


def clamp_var(v):
    with np.errstate(invalid="ignore"):
        return np.where(~(v < temporal_ref.VCAP), temporal_ref.VCAP, np.where(v > 0, v, np.float32(0))).astype(np.float32)


@pytest.mark.parametrize("w,h", SIZES)
def test_a_static_sequence_is_the_running_mean(w, h):
    """alpha_min = 0, n_max = +inf, one camera, 4 steps of 8 spp on synthetic guides (unit normals, so every hit accepts its own
    record): step k is N = 8k, al = f32(8 / N), c = fma(al, c_k - c, c), v = fma(al·al, s_k, ((1 - al)·(1 - al))·v) on hits, and the
    input on background pixels — in numpy, with the fma evaluated exactly."""
    frames = cases.plane_sequence(w, h, 17 * w + h, [(0, 0)] * 4)
    m = temporal_ref.Temporal(w, h)
    hit = frames[0]["index"] >= 0
    c = v = None
    for k, f in enumerate(frames, 1):
        got = frame_step(m, f, alpha_min=0.0, n_max=INF)
        assert m.last_static == (k > 1)
        s = clamp_var(f["var"])
        if k == 1:
            c, v = f["rgb"].copy(), s
        else:
            al = np.float32(8) / np.float32(8 * k)
            kk = np.float32(1) - al
            full = lambda x: np.full(c.shape, x, np.float32)  # noqa: E731
            cn = fma32(full(al), f["rgb"] - c, c)
            vn = fma32(full(al * al), s, (kk * kk) * v)
            c, v = np.where(hit[..., None], cn, f["rgb"]), np.where(hit[..., None], vn, s)
        same_bits(got[0], c, f"{w}x{h} step {k} colour")
        same_bits(got[1], v, f"{w}x{h} step {k} variance")
        same_bits(got[2], np.where(hit, np.float32(8 * k), np.float32(8)).astype(np.float32), f"{w}x{h} step {k} length")


@pytest.mark.parametrize("w,h", SIZES)
@pytest.mark.parametrize("kx,ky", [(1, 0), (0, 2), (2, 1)])
def test_an_integer_shift_is_numpy_slicing(w, h, kx, ky):
    """Frame 2's camera is frame 1's with px_origin moved by (-kx, -ky) on one synthetic world: pixel (px, py) takes the history of
    (px - kx, py - ky) — the output of step 1, sliced — with al = 1/2 (8 of 16 samples), where that pixel exists and is a hit; the input
    elsewhere.  fma(1/2, c - h, h) is (c - h)/2 + h in f32 ((c - h)/2 is exact), so numpy states it without an fma."""
    a, b = cases.plane_sequence(w, h, 31 * w + h + kx, [(kx, ky), (0, 0)])
    m = temporal_ref.Temporal(w, h)
    o1 = frame_step(m, a, alpha_min=0.0, n_max=INF)
    o2 = frame_step(m, b, alpha_min=0.0, n_max=INF)
    assert not m.last_static
    s = clamp_var(b["var"])
    want_c, want_v, want_n = b["rgb"].copy(), s.copy(), np.full((h, w), 8, np.float32)
    hit = b["index"] >= 0
    if w > kx and h > ky:
        hc, hv = o1[0][:h - ky, :w - kx], o1[1][:h - ky, :w - kx]
        sel = hit[ky:, kx:]
        assert np.array_equal(b["index"][ky:, kx:], a["index"][:h - ky, :w - kx])  # one world: the same hittables
        half, quarter = np.float32(0.5), np.float32(0.25)
        want_c[ky:, kx:][sel] = ((b["rgb"][ky:, kx:] - hc) * half + hc)[sel]
        vv = fma32(np.full(hv.shape, quarter), s[ky:, kx:], quarter * hv)
        want_v[ky:, kx:][sel] = vv[sel]
        want_n[ky:, kx:][sel] = 16
    same_bits(o2[0], want_c, "colour")
    same_bits(o2[1], want_v, "variance")
    same_bits(o2[2], want_n, "length")


def test_a_fractional_and_a_general_sequence_stay_finite_and_find_history():
    """The sequences the GPU test compares bit for bit: finite for every odd variance, and the moved step finds history."""
    for frames in (cases.plane_sequence(45, 23, 9, [(0, 0), (0, 0), (0.25, -0.625)]), cases.general_sequence(45, 23, 4)):
        m = temporal_ref.Temporal(45, 23)
        for f in frames:
            rgb, var, length = frame_step(m, f)
            assert np.isfinite(rgb).all() and np.isfinite(var).all() and (var >= 0).all() and (length >= 8).all()
        hit = frames[-1]["index"] >= 0
        assert not m.last_static and (length[hit] > 8).mean() > 0.5 and (length[~hit] == 8).all()


def test_the_contract_meets_what_the_end_to_end_test_asks(oracle):
    """What tests/test_temporal_gpu.py asserts on the device, on the CPU restatement first: threeSpheres at 64x36, oracle frames of 8 spp
    with a seed per frame (the oracle's frames are the device's, bit for bit), the first-hit G-buffer from tests/query_reference.py,
    static for three frames and then a pan of 1.5 pixels per frame, the defaults.  While static the length is 8·k; under the pan more
    than half of the hit pixels find history; and from the second frame on the accumulated frame is nearer the 512-spp frame of the
    same camera than the raw frame is.  (The colour does not depend on the variance fed in, so a constant stands in for the estimate.)"""
    import query_reference as qr
    from rayz_amd import tracer

    t = tracer.threeSpheres(64, seed=3)
    t.samples_per_px, t.max_bounces = 8, 8
    t.set_gpu(render_seed=17, chunk_spp=4, traversal=capi.TRAVERSAL_BVH, tmin=1e-3)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    w, h = p.width, p.height
    gx, gy = np.meshgrid(np.arange(w), np.arange(h))
    m = temporal_ref.Temporal(w, h)
    refs, shares, ratios = {}, [], []
    for k in range(6):
        pan = 1.5 * max(0, k - 2)
        c = capi.CameraDesc.from_buffer_copy(cam)
        for j in range(3):
            c.px_origin[j] = cam.px_origin[j] + pan * cam.px_du[j]
        lf, du, dv, po = (np.array(list(getattr(c, f))) for f in ("look_from", "px_du", "px_dv", "px_origin"))
        rays = np.zeros((h * w, 8))
        rays[:, 0:3], rays[:, 7] = lf, np.inf
        rays[:, 4:7] = (po[None, None] + gx[..., None] * du + gy[..., None] * dv - lf).reshape(-1, 3)
        rays = rays.astype(np.float32).astype(np.float64)
        idx, _, rec, _ = qr.brute_force(oracle, sd, rays, 1e-3, capi.PRECISION_F32)
        idx = idx.reshape(h, w).astype(np.int32)
        normal, point = (rec[:, a:a + 3].reshape(h, w, 3).astype(np.float32) for a in (5, 2))
        if pan not in refs:
            p.samples_per_px, p.chunk_spp, p.seed = 512, 0, 999
            refs[pan] = oracle.render_b(sd, c, p)[0].astype(np.float64)
        p.samples_per_px, p.chunk_spp, p.seed = 8, 4, 100 + k
        raw = oracle.render_b(sd, c, p)[0].astype(np.float32)
        out, var, length = m.step(raw, np.full((h, w, 3), 0.01, np.float32), idx, normal, point, c, 8)
        hit = idx >= 0
        assert hit.any() and np.isfinite(out).all() and np.isfinite(var).all()
        if k < 3:
            assert (length[hit] == 8 * (k + 1)).all()
        else:
            shares.append((length[hit] > 8).mean())
        if k:
            ratios.append(((out - refs[pan]) ** 2).mean() / ((raw - refs[pan]) ** 2).mean())
    print("share of hit pixels with history under the pan:", shares, "; temporal / raw MSE, frames 1..5:", ratios)
    assert min(shares) > 0.5 and max(ratios) < 1.0


# ---- the binding --------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayz_hip.h")).read(), flags=re.S)


def test_struct_layout_and_defaults_match_the_header(built):
    m = re.search(r"typedef struct RayzTemporalParams \{(.*?)\} RayzTemporalParams;", _header(), flags=re.S)
    names = [d.split()[1] for d in m.group(1).split(";") if d.split()]
    assert all(d.split()[0] == "double" for d in m.group(1).split(";") if d.split())
    assert names == ["alpha_min", "n_max", "normal_cos_min", "max_rel_dist"] == [n for n, _ in capi.TemporalParams._fields_]
    assert all(t is C.c_double for _, t in capi.TemporalParams._fields_) and C.sizeof(capi.TemporalParams) == 32
    hdr = _header()
    for k, v in capi.TEMPORAL_DEFAULTS.items():
        assert float(re.search(rf"RAYZ_TEMPORAL_DEFAULT_{k.upper()} (\S+)", hdr).group(1)) == v == temporal_ref.DEFAULTS[k]


def test_prototypes_in_header_and_binding(built):
    hdr = " ".join(_header().split())
    assert "int rayz_hip_temporal_create(int device, uint32_t width, uint32_t height, RayzTemporal** out);" in hdr
    assert ("int rayz_hip_temporal_step(RayzTemporal* tm, const RayzTemporalParams* params_or_null, const RayzCameraDesc* camera, uint32_t spp, "
            "const float* d_rgb_in, const float* d_var_rgb, const RayzQueryOutputs* gbuffer, float* d_rgb_out, float* d_var_out, "
            "float* d_length_out_or_null, void* hip_stream);") in hdr
    for tail in ("reset(RayzTemporal* tm);", "timing(RayzTemporal* tm, float* ms);", "destroy(RayzTemporal* tm);"):
        assert "int rayz_hip_temporal_" + tail in hdr
    protos = {p[0]: p for p in capi.PROTOTYPES}
    assert [len(protos["rayz_hip_temporal_" + k][2]) for k in ("create", "step", "reset", "timing", "destroy")] == [4, 11, 1, 2, 1]
    lib = capi.load()
    assert all(hasattr(lib, "rayz_hip_temporal_" + k) for k in ("create", "step", "reset", "timing", "destroy"))
    assert lib.rayz_hip_abi_version() == capi.ABI_VERSION == 5


def test_every_bad_argument_is_refused_before_the_handle(built):
    """All arguments are checked before the handle and nothing touches a device: with valid arguments and a null handle the answer is
    RAYZ_ERR_STATE, with any one bad argument RAYZ_ERR_BAD_ARG and a message that names it."""
    lib = capi.load()
    buf = C.c_void_p(4096)  # never dereferenced: the handle is refused first
    g = capi.QueryOutputs(index=4096, normal=4096, point=4096)
    good = capi.CameraDesc(look_from=(0, 0, -8), px_du=(1, 0, 0), px_dv=(0, 1, 0), px_origin=(0, 0, 0))

    def run(prm=None, cam=good, spp=8, rgb=buf, var=buf, gb=g, out=buf, vout=buf, length=None, **over):
        p = capi.TemporalParams(**{**capi.TEMPORAL_DEFAULTS, **over}) if prm is None else prm
        return lib.rayz_hip_temporal_step(None, C.byref(p) if p is not False else None, C.byref(cam) if cam is not None else None, spp, rgb,
                                          var, C.byref(gb) if gb is not None else None, out, vout, length, None)

    assert run() == capi.ERR_STATE and b"not a temporal handle" in lib.rayz_hip_last_error()
    assert run(prm=False) == capi.ERR_STATE  # NULL params: the defaults pass the checks
    assert run(length=buf) == capi.ERR_STATE and run(spp=1) == capi.ERR_STATE and run(spp=1 << 24) == capi.ERR_STATE
    assert run(alpha_min=0.0, n_max=INF, normal_cos_min=-1.0, max_rel_dist=INF) == capi.ERR_STATE
    assert run(alpha_min=1.0, n_max=1.0, normal_cos_min=1.0, max_rel_dist=1e-30) == capi.ERR_STATE
    bad = [(dict(alpha_min=-0.01), b"alpha_min"), (dict(alpha_min=1.01), b"alpha_min"), (dict(alpha_min=NAN), b"alpha_min"),
           (dict(n_max=0.5), b"n_max"), (dict(n_max=NAN), b"n_max"), (dict(n_max=-INF), b"n_max"),
           (dict(normal_cos_min=-1.5), b"normal_cos_min"), (dict(normal_cos_min=1.5), b"normal_cos_min"), (dict(normal_cos_min=NAN), b"normal_cos_min"),
           (dict(max_rel_dist=0.0), b"max_rel_dist"), (dict(max_rel_dist=-1.0), b"max_rel_dist"), (dict(max_rel_dist=NAN), b"max_rel_dist"),
           (dict(spp=0), b"spp"), (dict(spp=(1 << 24) + 1), b"spp")]
    for over, word in bad:
        assert run(**over) == capi.ERR_BAD_ARG, over
        assert word in lib.rayz_hip_last_error(), (over, lib.rayz_hip_last_error())
    for missing in ("rgb", "var", "out", "vout", "gb", "cam"):
        assert run(**{missing: None}) == capi.ERR_BAD_ARG, missing
    for field in ("index", "normal", "point"):
        part = capi.QueryOutputs(**{k: 4096 for k in ("index", "normal", "point", "albedo") if k != field})
        assert run(gb=part) == capi.ERR_BAD_ARG and b"index, normal and point" in lib.rayz_hip_last_error()
    # a camera without a volume: px_dv parallel to px_du, the lens centre in the pixel plane, a NaN, an overflowing det
    cams = [capi.CameraDesc(look_from=(0, 0, -8), px_du=(1, 0, 0), px_dv=(2, 0, 0), px_origin=(0, 0, 0)),
            capi.CameraDesc(look_from=(0, 0, 0), px_du=(1, 0, 0), px_dv=(0, 1, 0), px_origin=(3, 4, 0)),
            capi.CameraDesc(look_from=(0, 0, NAN), px_du=(1, 0, 0), px_dv=(0, 1, 0), px_origin=(0, 0, 0)),
            capi.CameraDesc(look_from=(0, 0, -1e200), px_du=(1e200, 0, 0), px_dv=(0, 1, 0), px_origin=(0, 0, 0)),
            capi.CameraDesc()]
    for cam in cams:
        assert run(cam=cam) == capi.ERR_BAD_ARG and b"det" in lib.rayz_hip_last_error()
    # the other entries refuse a handle that is none (destroy(NULL) is a no-op, as for every handle)
    assert lib.rayz_hip_temporal_reset(None) == capi.ERR_STATE and lib.rayz_hip_temporal_timing(None, None) == capi.ERR_STATE
    assert lib.rayz_hip_temporal_destroy(None) == capi.OK
    out = C.c_void_p(1)
    assert lib.rayz_hip_temporal_create(0, 0, 4, C.byref(out)) == capi.ERR_BAD_ARG and not out.value
    assert lib.rayz_hip_temporal_create(0, 1 << 16, 1 << 15, C.byref(out)) == capi.ERR_BAD_ARG and b"MAX_PIXELS" in lib.rayz_hip_last_error()
    assert lib.rayz_hip_temporal_create(0, 4, 4, None) == capi.ERR_BAD_ARG
