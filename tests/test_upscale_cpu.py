"""Guided upscaling without a GPU: the CPU restatement (tests/upscale_mirror.cpp, which the GPU tests hold the
kernels to bit for bit) on the hand cases of tests/upscale_cases.py — closed-form answers worked out in Fractions from surface
labels —, the stage coverage of the synthetic scenes the GPU tests run, partition of unity, the low-resolution camera and params,
and the C ABI: symbols, struct layout, and every refusal that needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import upscale_cases
import upscale_ref
import upscale_scenes
from rayz_amd import capi, render, tracer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = upscale_cases.cases()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def run_case(c):
    return upscale_ref.upscale(c["rgb_lo"], c["g_lo"], c["g_hi"], c["f"], var_rgb=c.get("var_lo"), flags=c.get("flags", 1))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_mirror_gives_the_hand_derived_answers(case):
    out, var, stage = run_case(case)
    want, want_var, want_stage = upscale_cases.expected(case)
    m = case.get("check", np.ones(stage.shape, bool))
    assert np.array_equal(stage[m], want_stage[m]), (stage, want_stage)
    assert np.array_equal(bits(out)[m], bits(want)[m]), (out[m], want[m])
    if want_var is not None:
        assert np.array_equal(bits(var)[m], bits(want_var)[m]), (var[m], want_var[m])
    # the closed form the case was built for, stated directly
    f, closed = case["f"], case["closed"]
    H, W = stage.shape
    if closed == "const":
        assert (stage == 0).all() and (out == np.float32(case["value"])).all()
    elif closed == "ramp_x":  # interior: (1 - fx)·c(i0) + fx·c(i0 + 1) = the ramp at the pixel's own position; clamped at the edges
        pos = np.clip(((np.arange(W) + 0.5) / f - 0.5), 0, W // f - 1)
        for ch, scale in enumerate((0.25, 0.5, 1.0)):
            assert (out[:, :, ch] == (pos * scale).astype(np.float32)[None, :]).all()
    elif closed == "corners":  # a corner pixel sees one tap: that pixel's colour; an edge pixel two: 1/4 and 3/4 along the edge
        lo = case["rgb_lo"]
        for (y, x), (j, i) in {(0, 0): (0, 0), (0, W - 1): (0, 2), (H - 1, 0): (2, 0), (H - 1, W - 1): (2, 2)}.items():
            assert (out[y, x] == lo[j, i]).all()
        assert out[0, 2, 0] == np.float32(0.25 * lo[0, 0, 0] + 0.75 * lo[0, 1, 0]) and out[0, 3, 0] == np.float32(0.75 * lo[0, 1, 0] + 0.25 * lo[0, 2, 0])
        assert out[3, 0, 0] == np.float32(0.75 * lo[1, 0, 0] + 0.25 * lo[2, 0, 0])
    elif closed == "two_planes":
        assert (out[:, :4] == np.float32((1.0, 0.0, 0.25))).all() and (out[:, 4:] == np.float32((0.0, 1.0, 0.5))).all() and (stage == 0).all()
    elif closed == "albedo":
        assert (out == np.float32(case["e"]) * case["g_hi"].albedo).all() and len(np.unique(out[..., 0])) == 2
    elif closed == "f3":
        assert (out[1::3, 1::3] == case["rgb_lo"]).all()
    elif closed == "background":
        assert (out[:, :4] == np.float32((0.5, 0.75, 1.0))).all()  # the sky: m = 1 whatever the albedo array holds
        assert (out[:, 4:] == np.float32((0.25, 0.5, 0.125))).all()  # e = c / (1/2), out = e·(1/2)
    elif closed == "var":  # Σb² / (Σb)²: 100/256 in the interior, 1 in a corner, 10/16 on an edge
        v = np.float32(case["v"])
        assert (var[2:4, 2:6] == v * np.float32(100 / 256)).all() and (var[0, 0] == v).all() and (var[0, 2] == v * np.float32(10 / 16)).all()
    elif closed == "stage1":
        assert (stage[:, 8] == 1).all() and (np.delete(stage, 8, axis=1) == 0).all()
        assert (out[:, 8] == np.float32((0.125, 1.0, 2.0))).all()
        # rows of the 4x4 footprint inside the frame: 4 in the interior (y = 3, 4), 3 next to the edge, 2 at y = 0 and y = 7
        assert (var[3, 8] == np.float32(0.25 / 4)).all() and (var[1, 8] == np.float32(0.25 / 3)).all() and (var[0, 8] == np.float32(0.25 / 2)).all()
    elif closed == "stage2":
        assert stage[2, 5] == 2 and stage.sum() == 2
        assert (out[2, 5] == case["rgb_lo"][1, 2]).all() and (var[2, 5] == upscale_ref.VCAP).all()
    else:
        raise AssertionError(closed)


def test_the_synthetic_scenes_reach_every_stage():
    """Over the sizes and factors tests/test_upscale_gpu.py runs, the mirror's stage map holds every stage at least once — and each
    factor does on its own."""
    seen = {f: set() for f in upscale_scenes.FACTORS}
    for f in upscale_scenes.FACTORS:
        for w, h in upscale_scenes.SIZES:
            s = upscale_scenes.synthetic_pair(w, h, f, seed=1)
            _, _, stage = upscale_ref.upscale(s["rgb_lo"], s["g_lo"], s["g_hi"], f, var_rgb=s["var_lo"])
            seen[f] |= set(np.unique(stage).tolist())
    assert all(v == {0, 1, 2} for v in seen.values()), seen


@pytest.mark.parametrize("f", [2, 4])
def test_partition_of_unity(f):
    """A constant demodulated colour e comes out as e·m_p exactly where W's terms are dyadic (f = 2 and 4: b is a multiple of 1/64;
    the guides of the hand cases: g is 0 or 1): stage 0 and stage 1 alike, whatever the full-size albedo."""
    lo = np.zeros((4, 8), np.int32)
    lo[:, 5] = 1
    hi = np.zeros((4 * f, 8 * f), np.int32)
    hi[:, 4 * f] = 1  # a strip two low-resolution columns left of the column that sees its plane: stage 1
    rng = np.random.default_rng(3)
    m_hi = np.exp2(-rng.integers(0, 6, hi.shape + (3,))).astype(np.float32)
    e = np.float32((0.75, 1.5, 0.3125))
    g_lo, g_hi = upscale_cases.guides(lo, f, 0.5), upscale_cases.guides(hi, 1, m_hi)
    rgb_lo = np.broadcast_to(e * np.float32(0.5), (4, 8, 3))
    out, _, stage = upscale_ref.upscale(rgb_lo, g_lo, g_hi, f)
    assert set(np.unique(stage).tolist()) == {0, 1}
    assert np.array_equal(bits(out), bits(e * m_hi))


@pytest.mark.parametrize("f", [2, 3, 4])
def test_lowres_camera_looks_at_the_block_centres(f):
    t = tracer.threeSpheres(48 * f, seed=1)
    cam, prm = t.camera_desc(), t.params()
    lo, lp = render.lowres_camera(cam, f), render.lowres_params(prm, f)
    assert (lp.width, lp.height) == (prm.width // f, prm.height // f)
    o, du, dv = (np.array(list(v), np.float64) for v in (cam.px_origin, cam.px_du, cam.px_dv))
    lo_o, lo_du, lo_dv = (np.array(list(v), np.float64) for v in (lo.px_origin, lo.px_du, lo.px_dv))
    i, j = np.meshgrid(np.arange(lp.width), np.arange(lp.height))
    centre = lo_o + i[..., None] * lo_du + j[..., None] * lo_dv
    mean = np.zeros_like(centre)
    for b in range(f):
        for a in range(f):
            mean += o + (f * i + a)[..., None] * du + (f * j + b)[..., None] * dv
    mean /= f * f
    scale = np.abs(mean).max()
    assert np.abs(centre - mean).max() <= 1e-12 * scale
    for k in ("look_from", "defocus_u", "defocus_v"):
        assert list(getattr(lo, k)) == list(getattr(cam, k))
    assert lo.defocus == cam.defocus and list(cam.px_du) != list(lo.px_du)


def test_lowres_params_refusals():
    t = tracer.threeSpheres(96, seed=1)
    p = t.params()
    assert (p.width, p.height) == (96, 54)
    q = render.lowres_params(p, 2)
    assert (q.width, q.height, q.samples_per_px, q.seed) == (48, 27, p.samples_per_px, p.seed) and (p.width, p.height) == (96, 54)
    for f in (4, 5, 0):  # 54 is no multiple of 4; 96 none of 5
        with pytest.raises(ValueError):
            render.lowres_params(p, f)
    for idx, cnt in ((0, 2), (1, 2), (1, 1)):
        s = capi.RenderParams.from_buffer_copy(p)
        s.shard_index, s.shard_count = idx, cnt
        with pytest.raises(ValueError, match="shard"):
            render.lowres_params(s, 2)


NAMES = ["rayz_hip_upscaler_" + k for k in ("create", "run", "timing", "destroy")]


def test_symbols_are_declared_exported_and_bound(built):
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "rayz_hip.h")).read()
    protos = {p[0]: p for p in capi.PROTOTYPES}
    for n in NAMES:
        assert re.search(r"\bint " + n + r"\(", hdr), n
        assert hasattr(lib, n) and n in protos, n
    assert [len(protos[n][2]) for n in NAMES] == [5, 10, 3, 1]
    assert C.sizeof(capi.UpscaleParams) == 24 and capi.UpscaleParams.sigma_plane.offset == 16 and capi.UpscaleParams.form.offset == 12
    assert lib.rayz_hip_abi_version() == 5
    assert "uint32_t factor;" in hdr and "uint32_t form;" in hdr


def _prm(**kw):
    return capi.UpscaleParams(**{"factor": 2, **capi.UPSCALE_DEFAULTS, "flags": capi.DENOISE_ALBEDO, **kw})


def _gb(base, drop=()):
    o = capi.QueryOutputs(index=base + (1 << 12), normal=base + (2 << 12), point=base + (3 << 12), albedo=base + (4 << 12))
    for k in drop:
        setattr(o, k, None)
    return o


def _run_rc(lib, prm="default", rgb=1 << 20, var=None, lo="ok", hi="ok", out=2 << 20, var_out=None, stage=None, handle=None):
    prm = _prm() if prm == "default" else prm
    lo = _gb(1 << 24) if lo == "ok" else lo
    hi = _gb(2 << 24) if hi == "ok" else hi
    return lib.rayz_hip_upscaler_run(handle, C.byref(prm) if prm is not None else None, C.c_void_p(rgb), C.c_void_p(var),
                                     C.byref(lo) if lo is not None else None, C.byref(hi) if hi is not None else None, C.c_void_p(out),
                                     C.c_void_p(var_out), C.c_void_p(stage), None)


def test_upscaler_refusals_without_a_device(built):
    """Every argument is checked before the handle, without touching a device: with good arguments and no handle the answer is
    RAYZ_ERR_STATE, with any one bad argument RAYZ_ERR_BAD_ARG and a message that names it.  (What can only be refused behind a
    live handle — a factor other than the handle's — is tests/test_upscale_gpu.py's.)"""
    lib = capi.load()
    h = C.c_void_p()
    for f in (0, 1, 5, 1 << 31):
        assert lib.rayz_hip_upscaler_create(-1, 64, 64, f, C.byref(h)) == capi.ERR_BAD_ARG and not h.value
        assert b"factor" in lib.rayz_hip_last_error()
    for wd, ht, f in ((10, 9, 2), (9, 10, 2), (8, 8, 3), (0, 8, 2), (8, 0, 4), (6, 9, 4)):
        assert lib.rayz_hip_upscaler_create(-1, wd, ht, f, C.byref(h)) == capi.ERR_BAD_ARG and not h.value
        assert b"multiple" in lib.rayz_hip_last_error()
    assert lib.rayz_hip_upscaler_create(-1, 1 << 16, 1 << 15, 2, C.byref(h)) == capi.ERR_BAD_ARG and b"MAX_PIXELS" in lib.rayz_hip_last_error()
    assert lib.rayz_hip_upscaler_create(-1, 8, 8, 2, None) == capi.ERR_BAD_ARG
    # good arguments: what is left to refuse is the handle
    junk = (C.c_uint32 * 64)()
    assert _run_rc(lib) == capi.ERR_STATE
    assert _run_rc(lib, handle=C.cast(junk, C.c_void_p)) == capi.ERR_STATE
    assert _run_rc(lib, var=3 << 20, var_out=4 << 20, stage=5 << 20) == capi.ERR_STATE
    assert _run_rc(lib, var=3 << 20) == capi.ERR_STATE  # a variance in with no variance out is allowed
    assert _run_rc(lib, _prm(flags=0), lo=_gb(1 << 24, ("albedo",)), hi=_gb(2 << 24, ("albedo",))) == capi.ERR_STATE
    for f in (2, 3, 4):
        assert _run_rc(lib, _prm(factor=f, normal_power_log2=16, form=capi.UPSCALE_FORM_DIRECT, sigma_plane=float("inf"))) == capi.ERR_STATE
    bad = [
        (None, b"params"), (_prm(factor=0), b"factor"), (_prm(factor=1), b"factor"), (_prm(factor=5), b"factor"),
        (_prm(normal_power_log2=17), b"normal_power_log2"), (_prm(flags=2), b"flag"), (_prm(flags=0x80000001), b"flag"), (_prm(form=2), b"form"),
        (_prm(sigma_plane=0.0), b"sigma_plane"), (_prm(sigma_plane=-0.25), b"sigma_plane"), (_prm(sigma_plane=float("nan")), b"sigma_plane"),
        (_prm(sigma_plane=1e-30), b"sigma_plane"),  # positive, but its f32 square is 0
    ]
    for prm, word in bad:
        assert _run_rc(lib, prm) == capi.ERR_BAD_ARG, word
        assert word in lib.rayz_hip_last_error(), (word, lib.rayz_hip_last_error())
    assert _run_rc(lib, rgb=None) == capi.ERR_BAD_ARG and _run_rc(lib, out=None) == capi.ERR_BAD_ARG
    assert _run_rc(lib, lo=None) == capi.ERR_BAD_ARG and _run_rc(lib, hi=None) == capi.ERR_BAD_ARG
    for k in ("index", "normal", "point"):
        for side in ("lo", "hi"):
            assert _run_rc(lib, **{side: _gb(3 << 24, (k,))}) == capi.ERR_BAD_ARG, (side, k)
            assert b"index, normal and point" in lib.rayz_hip_last_error()
    for side in ("lo", "hi"):  # the ALBEDO flag without albedo in either G-buffer
        assert _run_rc(lib, **{side: _gb(3 << 24, ("albedo",))}) == capi.ERR_BAD_ARG and b"albedo" in lib.rayz_hip_last_error()
    assert _run_rc(lib, var_out=4 << 20) == capi.ERR_BAD_ARG and b"variance" in lib.rayz_hip_last_error()  # var_out without var_in
    # an output that is an input, or another output
    lo, hi = _gb(1 << 24), _gb(2 << 24)
    for out in (1 << 20, lo.index, lo.normal, lo.point, lo.albedo, hi.index, hi.normal, hi.point, hi.albedo):
        assert _run_rc(lib, out=out) == capi.ERR_BAD_ARG and b"aliases" in lib.rayz_hip_last_error(), hex(out)
    assert _run_rc(lib, var=3 << 20, out=3 << 20) == capi.ERR_BAD_ARG and b"aliases" in lib.rayz_hip_last_error()
    assert _run_rc(lib, var=3 << 20, var_out=3 << 20) == capi.ERR_BAD_ARG and b"aliases" in lib.rayz_hip_last_error()
    assert _run_rc(lib, var=3 << 20, var_out=2 << 20) == capi.ERR_BAD_ARG and b"aliases" in lib.rayz_hip_last_error()
    assert _run_rc(lib, stage=hi.normal) == capi.ERR_BAD_ARG and _run_rc(lib, stage=2 << 20) == capi.ERR_BAD_ARG
    assert _run_rc(lib, _prm(flags=0), out=hi.albedo) == capi.ERR_STATE  # not read without the flag: no input
    assert lib.rayz_hip_upscaler_destroy(C.cast(junk, C.c_void_p)) == capi.ERR_STATE and lib.rayz_hip_upscaler_destroy(None) == capi.OK
    a, b = C.c_float(), C.c_float()
    assert lib.rayz_hip_upscaler_timing(None, C.byref(a), C.byref(b)) == capi.ERR_STATE
    assert lib.rayz_hip_upscaler_timing(C.cast(junk, C.c_void_p), C.byref(a), C.byref(b)) == capi.ERR_STATE


def test_create_needs_a_device(built):
    import torch

    lib = capi.load()
    h = C.c_void_p()
    rc = lib.rayz_hip_upscaler_create(0, 16, 16, 4, C.byref(h))
    if torch.cuda.is_available():
        assert rc == capi.OK and h.value and lib.rayz_hip_upscaler_destroy(h) == capi.OK
    else:
        assert rc == capi.ERR_NO_DEVICE and not h.value
