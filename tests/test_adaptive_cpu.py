"""Adaptive passes without a GPU: the restatement against answers worked by hand, and the interface —
symbols, refusals, the Zig text, the ABI version."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adaptive_cases as cases
import adaptive_ref
from rayz_amd import capi, render

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["rayz_hip_progressive_set_adaptive", "rayz_hip_progressive_adaptive_step", "rayz_hip_progressive_adaptive_step_f64",
       "rayz_hip_progressive_run_adaptive", "rayz_hip_progressive_run_adaptive_f64", "rayz_hip_progressive_sample_counts",
       "rayz_hip_progressive_frozen_at", "rayz_hip_adaptive_kat"]


def same(a, b):  # equal, a NaN equal to a NaN
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


@pytest.mark.parametrize("f64", [False, True])
def test_the_restatement_gives_the_hand_worked_answers(f64):
    r = adaptive_ref.run(cases.SUMS, cases.SIZES, cases.PASS_ENDS, f64=f64, **cases.PARAMS)
    assert r["frozen_at"].tolist() == cases.WANT_FROZEN_AT
    assert r["counts"].tolist() == cases.WANT_COUNTS
    assert same(r["frame"][:, 0], cases.WANT_RED) and (r["frame"][:, 1:] == 0).all()
    assert same(r["acc"][:, 0], cases.WANT_ACC_RED) and same(r["Q"][:, 0], cases.WANT_Q_RED)
    assert [l.tolist() for l in r["lists"]] == cases.WANT_LISTS
    # the frozen value of pixel 5 differs from the mean of its whole schedule; the never-frozen pixel 2 IS that mean
    assert r["frame"][5, 0] == 1.0 != cases.FULL_MEAN_RED_5 == cases.SUMS[:, 5, 0].sum() / sum(cases.SIZES)
    assert r["frame"][2, 0] == cases.SUMS[:, 2, 0].sum() / sum(cases.SIZES)


def test_pixel_1_freezes_at_two_chunks_once_min_chunks_allows_it():
    r = adaptive_ref.run(cases.SUMS, cases.SIZES, cases.PASS_ENDS, **{**cases.PARAMS, "min_chunks": 2})
    assert r["frozen_at"].tolist() == [3, 2, 0, 0, 2, 2] and r["frame"][1, 0] == 1.0 and r["counts"][1] == 4
    assert [l.tolist() for l in r["lists"]][:3] == [[0, 1, 2, 3, 4, 5], [0, 2, 3], [2, 3]]


def test_a_run_that_ends_early_moves_no_cursor():
    sums = np.ones((4, 5, 3))
    r = adaptive_ref.run(sums, [1, 1, 1, 1], [1, 2, 3, 4], min_chunks=2)
    assert r["frozen_at"].tolist() == [2] * 5 and r["chunks_done"] == 2 and [len(l) for l in r["lists"]] == [5, 5, 0, 0, 0]
    assert (r["frame"] == 1.0).all() and r["counts"].tolist() == [2] * 5


def test_deal_order_is_place_items():
    """The order a shard's pixels are dealt in, written out for 16x10: tile (0,0), tile (0,1), then rows 8 and 9."""
    got = adaptive_ref.deal_order(160, 16)
    want = [r * 16 + c0 + c for c0 in (0, 8) for r in range(8) for c in range(8)] + list(range(128, 160))
    assert got.tolist() == want and sorted(got.tolist()) == list(range(160))
    assert adaptive_ref.deal_order(30, 10).tolist() == list(range(30))  # width % 8 != 0: rows as they come
    assert adaptive_ref.deal_order(7).tolist() == list(range(7))


def test_symbols_are_exported_and_bound(built):
    lib = capi.load()
    bound = {p[0] for p in capi.PROTOTYPES}
    header = open(os.path.join(ROOT, "include", "rayz_hip.h")).read()
    for n in NEW:
        assert hasattr(lib, n) and n in bound and re.search(r"\b%s\(" % n, header), n
    assert C.sizeof(capi.AdaptiveSummary) == 40
    assert lib.rayz_hip_abi_version() == capi.ABI_VERSION == 5


def test_refusals_without_a_device(built):
    lib = capi.load()
    sm, prm = capi.AdaptiveSummary(), capi.NoiseParams(0.05, 0.02)
    assert lib.rayz_hip_progressive_set_adaptive(None, 4) == capi.ERR_STATE
    assert lib.rayz_hip_progressive_set_adaptive(None, 1) == capi.ERR_BAD_ARG and b"min_chunks" in lib.rayz_hip_last_error()
    for fn in (lib.rayz_hip_progressive_adaptive_step, lib.rayz_hip_progressive_adaptive_step_f64,
               lib.rayz_hip_progressive_run_adaptive, lib.rayz_hip_progressive_run_adaptive_f64):
        assert fn(None, C.byref(prm), 0, None, C.byref(sm), None) == capi.ERR_STATE
        assert fn(None, None, 0, None, None, None) == capi.ERR_STATE
        for bad in (capi.NoiseParams(0.0, 0.02), capi.NoiseParams(float("nan"), 0.02), capi.NoiseParams(0.05, -1.0)):
            assert fn(None, C.byref(bad), 0, None, C.byref(sm), None) == capi.ERR_BAD_ARG
    assert lib.rayz_hip_progressive_sample_counts(None, None, None) == capi.ERR_STATE
    assert lib.rayz_hip_progressive_frozen_at(None, None, None) == capi.ERR_STATE
    U, D = C.POINTER(C.c_uint32), C.POINTER(C.c_double)
    sums, sizes, ends = np.ones(6), np.array([1, 1], dtype=np.uint32), np.array([1, 2], dtype=np.uint32)
    def kat(precision=0, sizes=sizes, n_chunks=2, ends=ends, n_passes=2, width=0, min_chunks=2, prm=prm, n_pixels=1):
        return lib.rayz_hip_adaptive_kat(precision, sums.ctypes.data_as(D), sizes.ctypes.data_as(U), n_pixels, n_chunks, ends.ctypes.data_as(U),
                                         n_passes, width, min_chunks, C.byref(prm), None, None, None, None, None, None)
    assert kat(min_chunks=1) == capi.ERR_BAD_ARG and b"min_chunks" in lib.rayz_hip_last_error()
    assert kat(precision=7) == capi.ERR_BAD_ARG
    assert kat(prm=capi.NoiseParams(-1.0, 0.02)) == capi.ERR_BAD_ARG
    assert kat(n_passes=0) == capi.ERR_BAD_ARG and kat(n_chunks=0) == capi.ERR_BAD_ARG
    assert kat(ends=np.array([2, 2], dtype=np.uint32)) == capi.ERR_BAD_ARG and b"pass_ends" in lib.rayz_hip_last_error()
    assert kat(ends=np.array([1, 3], dtype=np.uint32)) == capi.ERR_BAD_ARG
    assert kat(sizes=np.array([1, 0], dtype=np.uint32)) == capi.ERR_BAD_ARG
    assert kat(n_pixels=3, width=2) == capi.ERR_BAD_ARG and b"whole rows" in lib.rayz_hip_last_error()
    with pytest.raises(ValueError):
        render.adaptive_kat(np.ones((2, 3)), [1, 1], [2])


def test_zig_text_carries_the_adaptive_interface():
    text = open(os.path.join(ROOT, "rayz_amd", "zig", "renderer_hip.zig")).read()
    for n in NEW:
        assert re.search(r"extern fn %s\(" % n, text), n
    m = re.search(r"pub const RayzAdaptiveSummary: type = extern struct \{(.*?)\n\};", text, flags=re.S)
    assert m, "RayzAdaptiveSummary"
    fields = re.findall(r"(\w+): (\w+)", re.sub(r"//.*", "", m.group(1)))
    assert fields == [("pixels", "u64"), ("active", "u64"), ("samples_traced", "u64"), ("passes", "u32"), ("chunks_done", "u32"),
                      ("samples_done", "u32"), ("_pad", "u32")]
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayz_hip.h")).read(), flags=re.S)
    c = re.search(r"typedef struct RayzAdaptiveSummary \{(.*?)\}", hdr, flags=re.S).group(1)
    ctype = {"uint64_t": "u64", "uint32_t": "u32"}
    assert [(n, ctype[t]) for t, n in re.findall(r"(\w+) (\w+);", c)] == fields
