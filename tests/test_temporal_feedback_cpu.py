"""Temporal accumulation's feedback mode on the CPU: the restatement tests/temporal_feedback_mirror.cpp equals the
moments mode's (tests/temporal_moments_mirror.cpp) bit for bit while no feedback is given, and its raw first moment then equals the
colour; feeding a step's own output back changes no record; the hand-derived answers of tests/temporal_feedback_cases.py, which
every named misreading of the section fails; the refusals of the new entry points that need no device; and the tap of the guided
filter, whose reference is the existing guided mirror at levels = t."""
import ctypes as C

import numpy as np
import pytest

import temporal_cases
import temporal_feedback_cases as cases
import temporal_feedback_ref as ref
import temporal_moments_ref
from rayz_amd import capi

SIZES = [(1, 1), (5, 3), (33, 9), (45, 23), (97, 41)]  # tests/test_temporal_moments_gpu.py's
ORIGINS = [(0, 0), (0, 0), (0.25, -0.625), (1.25, 0.375)]
PARAMS = [{}, dict(w2_max=0.0), dict(w2_max=1.0), dict(min_taps=2.0), dict(min_taps=49.0)]
GENERAL = PARAMS + [dict(alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)]
NAMES = ("colour", "variance", "length", "W2")


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ; first at {bad[:5].tolist()}"


def frame_args(f):
    return f["rgb"], f["index"], f["normal"], f["point"], f["camera"]


def sequences(w, h):
    yield "plane", temporal_cases.plane_sequence(w, h, 100 * w + h, ORIGINS), PARAMS
    yield "general", temporal_cases.general_sequence(w, h, 5 * w + h), GENERAL


@pytest.mark.parametrize("w,h", SIZES)
def test_without_feedback_the_mirror_is_the_moments_mirror(w, h):
    """All four outputs of every step, and the records c, g, p and m it leaves, equal the moments mirror's bit for bit; the m1 record
    is the colour record's rgb with 0 in its fourth slot (the moments mirror keeps its variance there, which nothing reads)."""
    for kind, frames, params in sequences(w, h):
        for prm in params:
            a, b = ref.TemporalFeedback(w, h), temporal_moments_ref.TemporalMoments(w, h)
            for k, f in enumerate(frames):
                got, want = a.step(*frame_args(f), 8, **prm), b.step(*frame_args(f), 8, **prm)
                for name, x, y in zip(NAMES, got, want):
                    same_bits(x, y, f"{w}x{h} {kind} {prm} step {k} {name}")
                sa, sb = a.state(), b.state()
                for r, name in ((0, "c"), (2, "g"), (3, "p"), (4, "m")):
                    same_bits(sa[r], sb[r], f"{w}x{h} {kind} {prm} step {k} record {name}")
                same_bits(np.ascontiguousarray(sa[1][..., :3]), np.ascontiguousarray(sa[0][..., :3]), f"{w}x{h} {kind} {prm} step {k} m1 against c")
                assert (sa[1][..., 3].view(np.uint32) == 0).all()


@pytest.mark.parametrize("w,h", SIZES[1:4])
def test_feeding_the_own_output_back_changes_nothing(w, h):
    for kind, frames, params in sequences(w, h):
        a, b = ref.TemporalFeedback(w, h), ref.TemporalFeedback(w, h)
        for k, f in enumerate(frames):
            got, want = a.step(*frame_args(f), 8), b.step(*frame_args(f), 8)
            before = a.state()
            a.feedback(got[0])
            for x, y, z in zip(a.state(), before, b.state()):
                assert x.tobytes() == y.tobytes() == z.tobytes(), (kind, k)
            for name, x, y in zip(NAMES, got, want):
                same_bits(x, y, f"{w}x{h} {kind} step {k} {name}")


def mirror_step(tm, s):
    return tm.step(s.rgb, s.index, s.normal, s.point, s.camera, s.spp, **s.params)


@pytest.mark.parametrize("case", cases.cases(), ids=lambda c: c.name)
def test_mirror_gives_the_hand_derived_answers(case):
    """Every case against its RATIONAL expectation."""
    h, w = case.steps[0].index.shape
    out = case.run(ref.TemporalFeedback(w, h), mirror_step, lambda tm, img: tm.feedback(img))
    case.check(*out, "mirror")


@pytest.mark.parametrize("variant", sorted(ref.VARIANTS), ids=lambda v: ref.VARIANTS[v].replace(" ", "-"))
def test_every_named_misreading_fails_a_hand_case(variant):
    failed = []
    for case in cases.cases():
        h, w = case.steps[0].index.shape
        out = case.run(ref.TemporalFeedback(w, h, variant=variant), mirror_step, lambda tm, img: tm.feedback(img))
        try:
            case.check(*out, ref.VARIANTS[variant])
        except AssertionError:
            failed.append(case.name)
    print(f"{ref.VARIANTS[variant]}: fails {failed}")
    assert failed, f"no hand case tells '{ref.VARIANTS[variant]}' from §4.17"


def test_the_misreading_b_names_gives_31_64():
    """The figure DESIGN.md §4.17 quotes for 'the variance from the returned colour' in case (B)."""
    case = cases.fed_back_once()
    out = case.run(ref.TemporalFeedback(1, 1, variant=1), mirror_step, lambda tm, img: tm.feedback(img))
    assert (out[1][0, 0] == np.float32(31 / 64)).all() and (out[0][0, 0] == np.float32(1 / 8)).all()


def test_feedback_without_history_is_refused_by_the_mirror():
    tm = ref.TemporalFeedback(2, 2)
    with pytest.raises(ValueError):
        tm.feedback(np.zeros((2, 2, 3), np.float32))


def test_refusals_that_need_no_device():
    """A null d_rgb, tap_level 0 or above `levels` (given and defaulted), a null tap and an aliased tap are RAYZ_ERR_BAD_ARG before
    the handle is looked at: the handle here is NULL, and no device is touched."""
    lib = capi.load()
    assert lib.rayz_hip_temporal_feedback(None, None, None) == capi.ERR_BAD_ARG
    assert b"null colour buffer" in lib.rayz_hip_last_error()
    buf = (C.c_float * 16)()
    a, b, c = (C.c_void_p(C.addressof(buf) + 4 * k) for k in (0, 4, 8))
    assert lib.rayz_hip_temporal_feedback(None, a, None) == capi.ERR_STATE  # (behind the argument: the handle)
    assert lib.rayz_hip_temporal_track_feedback(None) == capi.ERR_STATE
    prm = capi.DenoiseGuidedParams(**{**capi.DENOISE_GUIDED_DEFAULTS, "levels": 3})
    o = capi.QueryOutputs()

    def tap(params, level, d_tap, d_in=a, d_out=b):
        return lib.rayz_hip_denoiser_run_guided_tap(None, params, d_in, a, C.byref(o), d_out, None, level, d_tap, None)

    for params, level in ((C.byref(prm), 0), (C.byref(prm), 4), (None, 0), (None, capi.DENOISE_GUIDED_DEFAULTS["levels"] + 1)):
        assert tap(params, level, c) == capi.ERR_BAD_ARG
        assert b"tap_level" in lib.rayz_hip_last_error()
    assert tap(C.byref(prm), 1, None) == capi.ERR_BAD_ARG and b"null tap" in lib.rayz_hip_last_error()
    assert tap(C.byref(prm), 1, a) == capi.ERR_BAD_ARG and b"neither" in lib.rayz_hip_last_error()
    assert tap(C.byref(prm), 1, b) == capi.ERR_BAD_ARG and b"neither" in lib.rayz_hip_last_error()
    assert tap(C.byref(prm), 3, b, d_in=a, d_out=b) == capi.ERR_BAD_ARG
    assert tap(C.byref(prm), 3, c) == capi.ERR_BAD_ARG and b"G-buffer" in lib.rayz_hip_last_error()  # a good tap: the next check speaks


def test_the_tap_on_the_cpu_is_the_guided_mirror_at_fewer_levels():
    """The tap's contract needs no new restatement: after t levels of a 4-level run the re-modulated colour (the mirror's
    `each_level`) is, bit for bit, what the guided mirror returns for levels = t — the reference the GPU test holds the device's tap
    to — and the levels differ, so a tap taken at the wrong level would show."""
    import denoise_guided_ref as g
    from denoise_cases import synthetic
    from denoise_guided_cases import guided_variance

    w, h = 21, 13
    rgb, index, normal, point, albedo = synthetic(w, h, 77)
    var = guided_variance(rgb, 5)
    taps = g.denoise(rgb, var, index, normal, point, albedo, levels=4, each_level=True)
    outs = [g.denoise(rgb, var, index, normal, point, albedo, levels=t)[0] for t in (1, 2, 3, 4)]
    for t, (tap, out) in enumerate(zip(taps, outs), 1):
        same_bits(tap[0], out, f"tap at level {t}")
    assert all(not np.array_equal(outs[i], outs[i + 1]) for i in range(3))
