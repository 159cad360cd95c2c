"""Temporal accumulation's clip mode on the CPU: the restatement tests/temporal_clip_mirror.cpp against the
hand-derived answers of tests/temporal_clip_cases.py; with gamma = +inf, and in OFF mode, against the mirrors of the plain, the
moments and the background steps, bit for bit, outputs and history, with an all-zero map; what the rule leaves alone; the
interface's text; and the refusals that need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import temporal_background_ref
import temporal_cases
import temporal_clip_cases as cases
import temporal_clip_ref as ref
import temporal_moments_ref
import temporal_ref
from rayz_amd import capi

SIZES = [(1, 1), (5, 3), (33, 9), (45, 23), (97, 41)]
BINDING = dict(alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)
INF = float("inf")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bits(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    bad = np.argwhere(a.view(np.uint32) != b.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} values differ, first at {bad[0].tolist()}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}"


def sequences(w, h):
    """name -> frames, every frame with its "spp"."""
    out = {"general": temporal_cases.general_sequence(w, h, 5 * w + h), "edge": temporal_cases.edge_sequence(w, h, 7 * w + h),
           "moving": temporal_cases.moving_sequence(w, h, 3 * w + h)}
    return {k: [dict(f, spp=f.get("spp", 8)) for f in v] for k, v in out.items()}


def plain(handle, f, **prm):
    return handle.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], f["spp"], **prm)


def moments(handle, f, **prm):
    return handle.step(f["rgb"], f["index"], f["normal"], f["point"], f["camera"], f["spp"], **prm)


def case_step(handle, s):
    handle.set_background(s.mode)
    handle.set_clip(s.clip, s.gamma, s.min_taps)
    if isinstance(handle, ref.Temporal):
        return handle.step(s.rgb, s.var, s.index, s.normal, s.point, s.camera, s.spp, **s.params)
    return handle.step(s.rgb, s.index, s.normal, s.point, s.camera, s.spp, **s.params)


def check_map(case, clipped, what):
    for p, want in case.clipped.items():
        assert clipped[p] == want, f"{case.name} {what}: pixel {p} clipped byte {clipped[p]}, want {want} ({case.why})"


@pytest.mark.parametrize("case", cases.cases(), ids=lambda c: c.name)
def test_mirror_gives_the_hand_derived_answers(case):
    h, w = case.steps[0].index.shape
    m = ref.Temporal(w, h)
    case.check(*case.run(m, case_step), "mirror")
    check_map(case, m.clipped, "mirror")


@pytest.mark.parametrize("case", cases.moments_cases(), ids=lambda c: c.name)
def test_moments_mirror_gives_the_hand_derived_answers(case):
    h, w = case.steps[0].index.shape
    m = ref.TemporalMoments(w, h)
    case.check(*case.run(m, case_step), "mirror")
    check_map(case, m.clipped, "mirror")


def test_the_ghost_tells_the_clip_from_the_off_step():
    """The ghost's frames through the mirror in both modes: the colour is 0 against 1/2 per unit wherever there is history, and the
    variance and the length are the same bits."""
    outs = []
    for mode in ("variance", "off"):
        case = cases.ghost(mode)
        outs.append(case.run(ref.Temporal(5, 4), case_step))
    (c_on, v_on, n_on), (c_off, v_off, n_off) = outs
    assert (c_on[:, 1:] == 0).all() and (c_off[:, 1:] == np.float32([0.5, 0.25, 1.0])).all()
    same_bits(c_on[:, 0], c_off[:, 0], "no history: the input in both modes")
    same_bits(v_on, v_off, "variance")
    same_bits(n_on, n_off, "length")


@pytest.mark.parametrize("w,h", SIZES)
def test_gamma_inf_and_off_are_the_existing_steps(w, h):
    """VARIANCE with gamma = +inf, and OFF, against tests/temporal_mirror.cpp, temporal_moments_mirror.cpp and (in both background
    modes) temporal_background_mirror.cpp: every output and every history record of every step bit for bit, at the defaults and with
    the parameters binding; the map all 0."""
    for name, frames in sequences(w, h).items():
        for prm in ({}, BINDING):
            for clip in (dict(clip="variance", gamma=INF), dict(clip="off")):
                pairs = [(ref.Temporal(w, h, **clip), temporal_ref.Temporal(w, h), plain),
                         (ref.TemporalMoments(w, h, **clip), temporal_moments_ref.TemporalMoments(w, h), moments)]
                for bg in ("input", "accumulate"):
                    pairs += [(ref.Temporal(w, h, bg, **clip), temporal_background_ref.Temporal(w, h, bg), plain),
                              (ref.TemporalMoments(w, h, bg, **clip), temporal_background_ref.TemporalMoments(w, h, bg), moments)]
                for mine, theirs, step in pairs:
                    for k, f in enumerate(frames):
                        what = f"{w}x{h} {name} {type(theirs).__module__} {clip} step {k}"
                        for x, y in zip(step(mine, f, **prm), step(theirs, f, **prm)):
                            same_bits(x, y, what + " output")
                        for x, y in zip(mine.state(), theirs.state()):
                            same_bits(x, y, what + " history")
                        assert not mine.clipped.any(), what


@pytest.mark.parametrize("moments_mode", [False, True])
@pytest.mark.parametrize("w,h", [(45, 23), (97, 41)])
def test_what_the_rule_leaves_alone(w, h, moments_mode):
    """VARIANCE at the defaults against OFF on the same frames, each handle on its own history: first and static steps are equal bit
    for bit with an all-zero map; in a moving step the length (moments: and W2) is equal everywhere; and as long as the two
    histories agree (the first moving step) every output of a pixel whose byte is 0 is equal, the colour differs at pixels whose
    byte is 1 and nowhere else, and the plain step's variance is equal everywhere.  Every sequence clips some pixels with history and
    leaves others."""
    make, step = (ref.TemporalMoments, moments) if moments_mode else (ref.Temporal, plain)
    for name, frames in sequences(w, h).items():
        for bg in ("input", "accumulate"):
            a, b = make(w, h, bg, clip="variance"), make(w, h, bg)
            agree, some, none = True, 0, 0
            for k, f in enumerate(frames):
                ra, rb = step(a, f), step(b, f)
                what = f"{w}x{h} {name} {bg} step {k}"
                same_bits(ra[2], rb[2], what + " length")
                if moments_mode:
                    same_bits(ra[3], rb[3], what + " W2")
                if k == 0 or a.last_static:
                    assert not a.clipped.any(), what
                if agree:
                    cl = a.clipped.astype(bool)
                    for x, y in zip(ra, rb):
                        same_bits(x[~cl], y[~cl], what + " outputs of unclipped pixels")
                    if not moments_mode:
                        same_bits(ra[1], rb[1], what + " the plain step's variance")
                    differs = (ra[0].view(np.uint32) != rb[0].view(np.uint32)).any(axis=2)  # (a clip of an ulp may vanish in the blend)
                    assert not (differs & ~cl).any() and (differs.any() or not cl.any()), what
                    found = ra[2] > f["spp"]
                    some, none = some + int(cl.sum()), none + int((found & ~cl).sum())
                    assert not (cl & ~found).any(), what + ": a pixel without history is flagged"
                agree = agree and not a.clipped.any()
            assert some and none, (name, bg, some, none)


def test_a_nan_history_passes_through_unclipped():
    """The ghost's frames with a NaN in the history of (1, 1): the pixel that takes it, (1, 2), has h = NaN, both comparisons are
    false: c_out is NaN as in OFF mode and its byte is 0, while its neighbours are clipped to 0."""
    case = cases.ghost("variance")
    case.steps[0].rgb[1, 1] = np.nan
    m = ref.Temporal(5, 4)
    out = case.run(m, case_step)
    assert np.isnan(out[0][1, 2]).all() and m.clipped[1, 2] == 0
    assert (out[0][1, 3] == 0).all() and m.clipped[1, 3] == 1


# ---- the binding --------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayz_hip.h")).read(), flags=re.S)


def test_prototypes_and_constants_agree(built):
    hdr = " ".join(_header().split())
    for s in ("int rayz_hip_temporal_set_clip(RayzTemporal* tm, uint32_t mode, const RayzTemporalClipParams* params_or_null, "
              "uint8_t* d_clipped_or_null);",
              "int rayz_hip_temporal_get_clip(RayzTemporal* tm, uint32_t* mode, RayzTemporalClipParams* params_or_null);",
              "#define RAYZ_TEMPORAL_CLIP_OFF 0u", "#define RAYZ_TEMPORAL_CLIP_VARIANCE 1u", "#define RAYZ_TEMPORAL_CLIP_DEFAULT_GAMMA 1.0",
              "#define RAYZ_TEMPORAL_CLIP_DEFAULT_MIN_TAPS 4.0",
              "typedef struct RayzTemporalClipParams { double gamma; double min_taps; } RayzTemporalClipParams;"):
        assert s in hdr, s
    assert capi.TEMPORAL_CLIP == {"off": 0, "variance": 1} == ref.CLIP_MODES
    assert capi.TEMPORAL_CLIP_DEFAULTS == {"gamma": 1.0, "min_taps": 4.0} == ref.CLIP_DEFAULTS
    assert [f[0] for f in capi.TemporalClipParams._fields_] == ["gamma", "min_taps"] and C.sizeof(capi.TemporalClipParams) == 16
    protos = {p[0]: p for p in capi.PROTOTYPES}
    assert protos["rayz_hip_temporal_set_clip"][1:] == (C.c_int, [C.c_void_p, C.c_uint32, C.POINTER(capi.TemporalClipParams), C.c_void_p])
    assert protos["rayz_hip_temporal_get_clip"][1:] == (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(capi.TemporalClipParams)])
    lib = capi.load()
    assert hasattr(lib, "rayz_hip_temporal_set_clip") and hasattr(lib, "rayz_hip_temporal_get_clip")
    assert lib.rayz_hip_abi_version() == capi.ABI_VERSION == 5


def test_refusals_before_a_device_is_touched(built):
    """A mode that is neither constant, a gamma that is not >= 0 (a NaN included) and a min_taps outside [2, 49] are RAYZ_ERR_BAD_ARG
    whatever the handle; with good arguments — gamma = +inf and 0 among them — a handle that is none is RAYZ_ERR_STATE.  (The
    refusals that need a live handle — feedback, cubic, counts steps, an aliased d_clipped — are in tests/test_temporal_clip_gpu.py.)"""
    lib = capi.load()
    P = capi.TemporalClipParams
    for bad in (2, 3, 0xFFFFFFFF):
        assert lib.rayz_hip_temporal_set_clip(None, bad, None, None) == capi.ERR_BAD_ARG
        assert b"clip mode" in lib.rayz_hip_last_error()
    for mode in (0, 1):
        for gamma in (-1.0, -0.0 - 1e-300, float("nan"), -INF):
            assert lib.rayz_hip_temporal_set_clip(None, mode, C.byref(P(gamma, 4.0)), None) == capi.ERR_BAD_ARG, gamma
            assert b"gamma" in lib.rayz_hip_last_error()
        for taps in (1.0, 1.999, 49.5, 50.0, float("nan"), INF):
            assert lib.rayz_hip_temporal_set_clip(None, mode, C.byref(P(1.0, taps)), None) == capi.ERR_BAD_ARG, taps
            assert b"min_taps" in lib.rayz_hip_last_error()
        for good in (None, P(0.0, 2.0), P(INF, 49.0), P(1.0, 4.0)):
            assert lib.rayz_hip_temporal_set_clip(None, mode, C.byref(good) if good else None, None) == capi.ERR_STATE
            assert lib.rayz_hip_temporal_set_clip(None, mode, C.byref(good) if good else None, C.c_void_p(4096)) == capi.ERR_STATE
            assert b"not a temporal handle" in lib.rayz_hip_last_error()
    mode, prm = C.c_uint32(7), P(5.0, 6.0)
    assert lib.rayz_hip_temporal_get_clip(None, C.byref(mode), C.byref(prm)) == capi.ERR_STATE and mode.value == 7 and prm.gamma == 5.0
    assert lib.rayz_hip_temporal_get_clip(None, None, None) == capi.ERR_STATE
