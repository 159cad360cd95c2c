"""Temporal accumulation's cubic resampling mode without a GPU: the new CPU restatement
(tests/temporal_cubic_mirror.cpp) in bilinear mode against the mirrors of §4.15 and §4.16, bit for bit; in cubic mode against the
hand-derived answers of tests/temporal_cubic_cases.py and against the f64 statement of tests/temporal_cubic_f64.py with its derived
bound, whose misreadings each fail a named case or leave the bound; the fixture on which both the cubic and the fallback population
are large; and the binding — constants, prototypes, and every refusal that can be made before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import temporal_cases
import temporal_cubic_cases as cases
import temporal_cubic_f64 as f64
import temporal_cubic_ref as ref
import temporal_moments_ref
import temporal_ref
from rayz_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(33, 9), (45, 23), (97, 41)]
BINDING = dict(alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ; first at {bad[:5].tolist()}"


def sequences(w, h):
    return {"plane": temporal_cases.plane_sequence(w, h, 100 * w + h, [(0, 0), (0, 0), (0.25, -0.625), (1.25, 0.375)]),
            "general": temporal_cases.general_sequence(w, h, 5 * w + h), "moving": temporal_cases.moving_sequence(w, h, 3 * w + h),
            "edge": temporal_cases.edge_sequence(w, h, 7 * w + h)}


@pytest.mark.parametrize("w,h", [(5, 3), (33, 9), (45, 23)])
def test_bilinear_mode_is_the_existing_mirrors_bit_for_bit(w, h):
    for name, frames in sequences(w, h).items():
        for prm in ({}, BINDING):
            old, new = temporal_ref.Temporal(w, h), ref.Temporal(w, h)
            oldm, newm = temporal_moments_ref.TemporalMoments(w, h), ref.TemporalMoments(w, h)
            for k, f in enumerate(frames):
                spp = f.get("spp", 8)
                a = old.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], spp, **prm)
                b = new.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], spp, **prm)
                for x, y, what in zip(a, b, ("colour", "variance", "length")):
                    same_bits(y, x, f"{name} {w}x{h} plain step {k} {what}")
                a = oldm.step(f["rgb"], f["index"], f["normal"], f["point"], f["camera"], spp, **prm)
                b = newm.step(f["rgb"], f["index"], f["normal"], f["point"], f["camera"], spp, **prm)
                for x, y, what in zip(a, b, ("colour", "variance", "length", "W2")):
                    same_bits(y, x, f"{name} {w}x{h} moments step {k} {what}")
                assert not new.taken.any() and not newm.taken.any()
            for x, y in zip(old.state() + oldm.state(), new.state() + newm.state()):
                same_bits(y, x, f"{name} {w}x{h} history")


def test_weights_are_the_exact_dyadics():
    for f, want in cases.WEIGHTS.items():
        assert cases.weights(f) == tuple(want), f
        got = ref.weights(float(f))
        assert [float(x) for x in got] == [float(x) for x in want], (f, got)
        assert sum(want) == 1
    assert np.signbit(ref.weights(0.0)[0]) and ref.weights(0.0)[1] == 1  # (-0, 1, 0, -0): an integer shift adds nothing


def plain_step(handle, s):
    return handle.step(s.rgb, s.var, s.index, s.normal, s.point, s.camera, s.spp, **s.params)


def moments_step(handle, s):
    return handle.step(s.rgb, s.index, s.normal, s.point, s.camera, s.spp, **s.params)


@pytest.mark.parametrize("case", cases.cases() + [f64.length_case(), f64.variance_case()], ids=lambda c: c.name)
def test_mirror_gives_the_hand_derived_answers(case):
    h, w = case.steps[0].index.shape
    m = ref.Temporal(w, h, "cubic")
    rgb, var, length = case.run(m, plain_step)
    case.check(rgb, var, length, "mirror")
    case.check_taken(m.taken, "mirror")


@pytest.mark.parametrize("case", cases.bilinear_cases(), ids=lambda c: c.name)
def test_mirror_in_bilinear_mode_misses_the_quadratic_by_the_closed_form(case):
    h, w = case.steps[0].index.shape
    for m in (ref.Temporal(w, h), temporal_ref.Temporal(w, h)):
        rgb, var, length = case.run(m, plain_step)
        case.check(rgb, var, length, "bilinear")
        assert not getattr(m, "taken", np.zeros(1)).any()


@pytest.mark.parametrize("case", cases.moments_cases(), ids=lambda c: c.name)
def test_mirror_gives_the_hand_derived_moments_answers(case):
    h, w = case.steps[0].index.shape
    m = ref.TemporalMoments(w, h, "cubic")
    case.check(*case.run(m, moments_step), "mirror")
    assert m.taken[2, 2] == 1


def run_blocks(w, h, handle):
    """The block sequence through `handle`; per moved step (taken, found history, hit)."""
    out = []
    for f in cases.block_sequence(w, h, 11 * w + h):
        res = handle.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], 8)
        if handle.has_history and handle.last_static is False and len(out) < 8 and res[2].max() > 8:
            hit = f["index"] >= 0
            out.append((handle.taken.astype(bool), (res[2] > 8) & hit, hit))
    return out


@pytest.mark.parametrize("w,h", SIZES)
def test_the_block_sequence_has_both_populations(w, h):
    """In every moved step, by the mirror alone: at least 20 % of the hit pixels that found history take the cubic path and at least
    5 % do not — so a comparison on this fixture cannot pass by comparing bilinear with bilinear, nor cubic with cubic."""
    moved = run_blocks(w, h, ref.Temporal(w, h, "cubic"))
    assert len(moved) == 2
    for taken, found, hit in moved:
        assert found.sum() > 0.5 * hit.sum() and not (taken & ~found).any()
        share = taken[found].mean()
        print(f"{w}x{h}: {found.sum()} pixels with history, {share:.3f} of them cubic")
        assert share >= 0.20 and 1 - share >= 0.05, (w, h, share)


@pytest.mark.parametrize("w,h", [(45, 23)])
def test_mirror_stays_within_the_f64_bound(w, h):
    """The cubic colours of the mirror against the f64 statement, on the block and the moving sequence: within the bound its
    docstring derives, and every misreading leaves it (or fails a hand case: test_every_misreading_is_caught)."""
    for name in ("blocks", "moving"):
        worst = f64.check_sequence(name, w, h)
        print(f"{name} {w}x{h}: worst error / bound {worst:.3f}")
        assert worst <= 1.0


def test_the_section_as_written_passes_every_case_and_sequence():
    assert f64.caught_by(None) == []


@pytest.mark.parametrize("switch", sorted(f64.SWITCHES))
def test_every_misreading_is_caught(switch):
    caught = f64.caught_by(switch)
    print(switch, "->", caught)
    assert caught, f"the misreading {switch!r} passes every hand case and stays inside the bound"


# ---- the binding --------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayz_hip.h")).read(), flags=re.S)


def test_prototypes_and_constants_agree(built):
    hdr = " ".join(_header().split())
    assert "int rayz_hip_temporal_set_resampling(RayzTemporal* tm, uint32_t mode, uint8_t* d_taken_or_null);" in hdr
    assert "int rayz_hip_temporal_get_resampling(RayzTemporal* tm, uint32_t* mode);" in hdr
    assert re.search(r"#define RAYZ_TEMPORAL_RESAMPLE_BILINEAR 0u", hdr) and re.search(r"#define RAYZ_TEMPORAL_RESAMPLE_CUBIC 1u", hdr)
    assert (capi.TEMPORAL_RESAMPLE_BILINEAR, capi.TEMPORAL_RESAMPLE_CUBIC) == (0, 1)
    assert capi.TEMPORAL_RESAMPLING == {"bilinear": 0, "cubic": 1} == ref.MODES
    protos = {p[0]: p for p in capi.PROTOTYPES}
    assert protos["rayz_hip_temporal_set_resampling"][1:] == (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p])
    assert protos["rayz_hip_temporal_get_resampling"][1:] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)])
    lib = capi.load()
    assert hasattr(lib, "rayz_hip_temporal_set_resampling") and hasattr(lib, "rayz_hip_temporal_get_resampling")
    assert lib.rayz_hip_abi_version() == capi.ABI_VERSION == 5


def test_refusals_before_a_device_is_touched(built):
    """A bad mode is RAYZ_ERR_BAD_ARG whatever the handle; a handle that is none is RAYZ_ERR_STATE.  (The refusals that need a live
    handle — counts steps, feedback, an aliased d_taken — are in tests/test_temporal_cubic_gpu.py.)"""
    lib = capi.load()
    mode = C.c_uint32(7)
    for bad in (2, 3, 0xFFFFFFFF):
        assert lib.rayz_hip_temporal_set_resampling(None, bad, None) == capi.ERR_BAD_ARG
        assert b"resampling mode" in lib.rayz_hip_last_error()
    for good in (0, 1):
        assert lib.rayz_hip_temporal_set_resampling(None, good, None) == capi.ERR_STATE
        assert lib.rayz_hip_temporal_set_resampling(None, good, C.c_void_p(4096)) == capi.ERR_STATE
        assert b"not a temporal handle" in lib.rayz_hip_last_error()
    assert lib.rayz_hip_temporal_get_resampling(None, C.byref(mode)) == capi.ERR_STATE and mode.value == 7
    assert lib.rayz_hip_temporal_get_resampling(None, None) == capi.ERR_STATE
