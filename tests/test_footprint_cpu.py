"""The footprint albedo without a GPU: the CPU restatement (tests/footprint_mirror.cpp, which the GPU tests hold
the kernel to bit for bit) on the hand cases of tests/footprint_cases.py; the capability it exists for — the upscale mirror
(tests/upscale_ref.py, §4.20 as it stands) fed the filtered albedo returns irradiance x full-size albedo EXACTLY where the
point-sampled albedo is off by the texture's contrast —; and the C ABI: symbols, and every refusal that needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import footprint_cases
import footprint_ref
import upscale_ref
from rayz_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = footprint_cases.cases()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def test_the_cases_the_issue_names_are_there():
    names = {c["name"] for c in CASES}
    assert {"checker_f2", "checker_f3", "checker_f4", "only_the_last_matches_f2", "all_match_f4", "background_beside_hits", "nothing_matches",
            "ramp_to_the_last_row_and_column_f2", "one_by_one_f2"} <= names
    assert {c["f"] for c in CASES} == {2, 3, 4}
    # f = 3's divide really rounds: 17/36 is no float32
    c = next(c for c in CASES if c["name"] == "checker_f3")
    assert footprint_cases.Fr(float(c["want"][0, 0, 0])) != footprint_cases.Fr(17, 36)


def test_round32_rounds_once_to_nearest_even():
    Fr, r = footprint_cases.Fr, footprint_cases.round32
    assert r(Fr(1, 3)) == np.float32(1.0) / np.float32(3.0) and r(Fr(-1, 3)) == -(np.float32(1.0) / np.float32(3.0))
    assert r(1 + Fr(1, 2 ** 24)) == np.float32(1.0)                     # a tie: to the even neighbour, down ..
    assert r(1 + Fr(3, 2 ** 24)) == np.float32(1.0) + np.float32(2.0 ** -22)  # .. and up
    assert r(1 + Fr(1, 2 ** 24) + Fr(1, 2 ** 60)) == np.float32(1.0) + np.float32(2.0 ** -23)  # just above a tie, where f64 first would tie
    assert r(0) == 0 and r(Fr(3, 16)) == np.float32(0.1875)


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_mirror_gives_the_hand_derived_answers(case):
    keep = {k: case[k].copy() for k in ("index_lo", "albedo_lo", "index_hi", "albedo_hi")}
    out, count = footprint_ref.footprint(case["index_lo"], case["albedo_lo"], case["index_hi"], case["albedo_hi"], case["f"])
    assert np.array_equal(count, case["want_count"]), (count, case["want_count"])
    assert np.array_equal(bits(out), bits(case["want"])), (out, case["want"])
    for k, v in keep.items():  # the inputs are untouched
        assert np.array_equal(bits(case[k]), bits(v)), k


def test_the_filtered_albedo_restores_the_texture_exactly():
    """★ With the footprint albedo as the low-resolution G-buffer's albedo and flags = DENOISE_ALBEDO, every full pixel of §4.20 comes
    out as E x albedo_hi[p] exactly (E is a power of two per channel: acc = E·W without a rounding).  With the point sample every
    pixel is off by the factor 2 (the ray saw A: 0.5 / 0.25) or 2/3 (it saw B: 0.5 / 0.75) in the channels the checker varies in."""
    c = footprint_cases.capability_case()
    f, E, a_hi = c["f"], c["E"], c["albedo_hi"]
    truth = E * a_hi
    lo = c["g_lo"](c["point_A"])
    filtered, count = footprint_ref.footprint_guides(lo, c["g_hi"], f)
    assert (count == 4).all() and (filtered == np.float32((0.5, 0.5, 0.25))).all()
    out, _, stage = upscale_ref.upscale(c["rgb_lo"], c["g_lo"](filtered), c["g_hi"], f, flags=upscale_ref.ALBEDO)
    assert (stage == 0).all() and np.array_equal(bits(out), bits(truth))
    assert len(np.unique(out[..., 0])) == 2  # the checker is back at full resolution
    # the flaw this removes
    out_a, _, _ = upscale_ref.upscale(c["rgb_lo"], lo, c["g_hi"], f, flags=upscale_ref.ALBEDO)
    assert np.array_equal(bits(out_a[..., 0]), bits(2 * truth[..., 0])) and np.array_equal(bits(out_a[..., 2]), bits(2 * truth[..., 2]))
    assert np.array_equal(bits(out_a[..., 1]), bits(truth[..., 1]))  # G is constant 1/2: no flaw to see there
    out_b, _, _ = upscale_ref.upscale(c["rgb_lo"], c["g_lo"](c["point_B"]), c["g_hi"], f, flags=upscale_ref.ALBEDO)
    for ch in (0, 2):
        ratio = out_b[..., ch].astype(np.float64) / truth[..., ch]
        assert np.abs(ratio - 2 / 3).max() <= 4 * 2.0 ** -24, ratio  # (c / m, the divide by W and the product round)


NAMES = ["rayz_hip_upscaler_footprint_albedo", "rayz_hip_upscaler_footprint_timing"]


def test_symbols_are_declared_exported_and_bound(built):
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "rayz_hip.h")).read()
    protos = {p[0]: p for p in capi.PROTOTYPES}
    for n in NAMES:
        assert re.search(r"\bint " + n + r"\(", hdr), n
        assert hasattr(lib, n) and n in protos, n
    assert [len(protos[n][2]) for n in NAMES] == [6, 2]
    assert lib.rayz_hip_abi_version() == 5  # additive within ABI 5
    assert capi.UPSCALE_DEFAULTS["flags"] == 0  # no default changed


def _gb(base, drop=()):
    o = capi.QueryOutputs(index=base + (1 << 12), albedo=base + (4 << 12))  # only index and albedo are required
    for k in drop:
        setattr(o, k, None)
    return o


def _rc(lib, lo="ok", hi="ok", out=2 << 20, count=None, handle=None):
    lo = _gb(1 << 24) if lo == "ok" else lo
    hi = _gb(2 << 24) if hi == "ok" else hi
    return lib.rayz_hip_upscaler_footprint_albedo(handle, C.byref(lo) if lo is not None else None, C.byref(hi) if hi is not None else None,
                                                  C.c_void_p(out), C.c_void_p(count), None)


def test_footprint_refusals_without_a_device(built):
    """Every argument is checked before the handle, without touching a device: with good arguments and no handle the answer is
    RAYZ_ERR_STATE, with any one bad argument RAYZ_ERR_BAD_ARG and a message that names it.  (An overlap that only the handle's
    sizes reveal is tests/test_footprint_gpu.py's.)"""
    lib = capi.load()
    junk = (C.c_uint32 * 64)()
    assert _rc(lib) == capi.ERR_STATE and b"upscaler" in lib.rayz_hip_last_error()
    assert _rc(lib, handle=C.cast(junk, C.c_void_p)) == capi.ERR_STATE
    assert _rc(lib, count=3 << 20) == capi.ERR_STATE
    assert _rc(lib, lo=None) == capi.ERR_BAD_ARG and b"G-buffer" in lib.rayz_hip_last_error()
    assert _rc(lib, hi=None) == capi.ERR_BAD_ARG and b"G-buffer" in lib.rayz_hip_last_error()
    assert _rc(lib, out=None) == capi.ERR_BAD_ARG and b"output" in lib.rayz_hip_last_error()
    for k in ("index", "albedo"):
        for side in ("lo", "hi"):
            assert _rc(lib, **{side: _gb(3 << 24, (k,))}) == capi.ERR_BAD_ARG, (side, k)
            assert b"index and albedo" in lib.rayz_hip_last_error()
    # normal and point are not needed (they are absent above); an output that is an input, or the other output
    lo, hi = _gb(1 << 24), _gb(2 << 24)
    for out in (lo.index, lo.albedo, hi.index, hi.albedo):  # lo.albedo: in place is refused as well
        assert _rc(lib, out=out) == capi.ERR_BAD_ARG and b"aliases" in lib.rayz_hip_last_error(), hex(out)
        assert _rc(lib, count=out) == capi.ERR_BAD_ARG and b"aliases" in lib.rayz_hip_last_error(), hex(out)
    assert _rc(lib, count=2 << 20) == capi.ERR_BAD_ARG and b"aliases" in lib.rayz_hip_last_error()
    # a bad argument wins over a bad handle; the order among the arguments: G-buffer, output, fields, aliases
    assert _rc(lib, lo=None, out=None, handle=C.cast(junk, C.c_void_p)) == capi.ERR_BAD_ARG and b"G-buffer" in lib.rayz_hip_last_error()
    assert _rc(lib, lo=_gb(3 << 24, ("index",)), out=None) == capi.ERR_BAD_ARG and b"output" in lib.rayz_hip_last_error()
    ms = C.c_float(-1.0)
    assert lib.rayz_hip_upscaler_footprint_timing(None, C.byref(ms)) == capi.ERR_STATE
    assert lib.rayz_hip_upscaler_footprint_timing(C.cast(junk, C.c_void_p), C.byref(ms)) == capi.ERR_STATE and ms.value == -1.0


def test_the_run_still_refuses_a_new_flag_bit(built):
    """The feature reaches rayz_hip_upscaler_run only as a better gbuffer_lo->albedo: RayzUpscaleParams.flags got no new bit."""
    lib = capi.load()
    prm = capi.UpscaleParams(**{"factor": 2, **capi.UPSCALE_DEFAULTS, "flags": 2})
    lo, hi = capi.QueryOutputs(index=1 << 12, normal=2 << 12, point=3 << 12, albedo=4 << 12), capi.QueryOutputs(index=5 << 12, normal=6 << 12, point=7 << 12, albedo=8 << 12)
    rc = lib.rayz_hip_upscaler_run(None, C.byref(prm), C.c_void_p(1 << 20), None, C.byref(lo), C.byref(hi), C.c_void_p(2 << 20), None, None, None)
    assert rc == capi.ERR_BAD_ARG and b"flag" in lib.rayz_hip_last_error()
