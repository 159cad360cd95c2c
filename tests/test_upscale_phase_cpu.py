"""Guided upscaling with a phase, without a device (rayz_hip_upscaler_run_phase; DESIGN.md §4.20 "Lattice samples"): the
restatement tests/upscale_phase_mirror.cpp against the hand cases' rational answers and their closed forms, against the restatement
of the run without a phase where the two position rules coincide (f = 3, phase (1, 1)), and the refusals decided before a handle."""
import ctypes as C

import numpy as np
import pytest

import upscale_phase_cases as cases
import upscale_ref
import upscale_scenes
from rayz_amd import capi

CASES = cases.cases()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


def run(c, **kw):
    return cases.upscale(c["rgb_lo"], c["g_lo"], c["g_hi"], c["f"], c["phase"], var_rgb=c.get("var_lo"), flags=c.get("flags", 1), **kw)


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_mirror_gives_the_rational_answers(c):
    out, var, stage = run(c)
    want, want_var, want_stage = cases.expected(c)
    m = c.get("check", np.ones(c["labels_hi"].shape, bool))
    assert np.array_equal(stage[m], want_stage[m])
    assert np.array_equal(bits(out)[m], bits(want)[m]), np.argwhere(bits(out)[m] != bits(want)[m])[:4]
    if want_var is not None:
        assert np.array_equal(bits(var)[m], bits(want_var)[m])


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_closed_forms(c):
    """What each case is about, stated without the tap arithmetic."""
    out, var, stage = run(c)
    f, (px, py) = c["f"], c["phase"]
    H, W = c["labels_hi"].shape
    h, w = H // f, W // f
    x, y = np.meshgrid(np.arange(W), np.arange(H))
    sampled = ((x - px) % f == 0) & ((y - py) % f == 0)
    kind = c["closed"]
    if kind == "const":
        assert (out == np.asarray(c["value"], np.float32)).all() and (stage == 0).all()
    elif kind == "ramp_x":
        # the ramp itself from the first sample to the last (i0 = -1 left of it, i0 + 1 = w right of it: the edge sample's value)
        want = cases.ramp(np.clip(x, px, f * (w - 1) + px))
        assert np.array_equal(bits(out), bits(want)) and (stage == 0).all()
        assert px == 0 or not np.array_equal(out[:, 0], cases.ramp(0)[None].repeat(H, 0))  # (left of the first sample it is NOT the ramp)
    elif kind == "corners":
        want = c["full"][np.clip(y, 1, 5), np.clip(x, 1, 5)]
        assert np.array_equal(bits(out), bits(want)) and (stage == 0).all()
        assert (out[0, 0] == c["full"][1, 1]).all()  # i0 = j0 = -1: one tap
    elif kind == "sampled":
        raw = np.zeros((H, W, 3), np.float32)
        raw[py::f, px::f] = c["rgb_lo"]
        assert np.array_equal(bits(out)[sampled], bits(raw)[sampled]) and (stage[sampled] == 0).all()
        v = np.zeros((H, W, 3), np.float32)
        v[py::f, px::f] = c["var_lo"]
        assert (var[sampled][np.isfinite(v[sampled]) & (v[sampled] > 0)] == np.float32(0.3)).all()
        assert (var[1, 2] == cases.VCAP).all() and var[3, 4, 0] == 0 and (var[5, 6] == cases.VCAP).all()  # +inf, -1, NaN
        # .. under both flag states, and it is NOT what interpolating the one tap gives with this albedo
        plain = cases.upscale(c["rgb_lo"], c["g_lo"], c["g_hi"], f, c["phase"], var_rgb=c["var_lo"], flags=0)
        assert np.array_equal(bits(plain[0])[sampled], bits(raw)[sampled])
        m = c["g_hi"].albedo
        assert not np.array_equal(bits((raw / m) * m)[sampled], bits(raw)[sampled])
    elif kind == "refused":
        assert sampled[2, 4] and stage[2, 4] == 1 and (out[2, 4] == np.float32((0.5, 0.25, 0.75))).all()
        assert (var[2, 4] == np.float32(0.25 * 8 / 64)).all()
        assert (stage[sampled & ~((x == 4) & (y == 2))] == 0).all() and (out[..., 0] <= 0.5).all()  # the other surface's 8.0 went nowhere
    elif kind == "stage2":
        assert stage[1, 3] == 2 and (stage == 2).sum() == 1
        assert (out[1, 3] == c["rgb_lo"][1, 2]).all() and (out[1, 3] != c["rgb_lo"][0, 1]).any() and (var[1, 3] == cases.VCAP).all()
    else:
        raise AssertionError(kind)


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (9, 5), (17, 9)])
@pytest.mark.parametrize("flags", [capi.DENOISE_ALBEDO, 0])
def test_f3_phase_11_is_the_block_centre_run_off_the_samples(w, h, flags):
    """At f = 3 the block centres ARE the lattice of phase (1, 1): both position rules name the same taps with the same weights
    ((2r) / (2f) and r / f are one quotient) and the same nearest sample, so the two restatements agree bit for bit at every pixel
    that is not a sample — and differ where the pass-through applies."""
    s = upscale_scenes.synthetic_pair(w, h, 3, seed=2)
    g_lo = cases.lattice(s["g_hi"], 3, (1, 1))
    for k in ("index", "normal", "point", "albedo"):  # the synthetic pair's low-resolution guides are that lattice's already
        assert np.array_equal(bits(getattr(g_lo, k)), bits(getattr(s["g_lo"], k))), k
    prm = dict(flags=flags, sigma_plane=0.3)
    old = upscale_ref.upscale(s["rgb_lo"], s["g_lo"], s["g_hi"], 3, var_rgb=s["var_lo"], **prm)
    new = cases.upscale(s["rgb_lo"], g_lo, s["g_hi"], 3, (1, 1), var_rgb=s["var_lo"], **prm)
    sampled = np.zeros((3 * h, 3 * w), bool)
    sampled[1::3, 1::3] = True
    for a, b, name in zip(old, new, ("colour", "variance", "stage map")):
        assert np.array_equal(bits(a)[~sampled], bits(b)[~sampled]), name
    # at the samples: the raw colour wherever the old run stayed in stage 0 (its one tap b = 1 was accepted with g > 0)
    passed = sampled & (old[2] == 0)
    raw = np.zeros_like(new[0])
    raw[1::3, 1::3] = s["rgb_lo"]
    assert passed.sum() >= 0.5 * sampled.sum() and np.array_equal(bits(new[0])[passed], bits(raw)[passed])
    assert np.array_equal(new[2][sampled], old[2][sampled])


def _gb(base):
    return capi.QueryOutputs(index=base + (1 << 12), normal=base + (2 << 12), point=base + (3 << 12), albedo=base + (4 << 12))


def test_run_phase_refusals_without_a_device(built):
    """The phase is checked with the other arguments, before the handle: good arguments and no handle give RAYZ_ERR_STATE."""
    lib = capi.load()
    lo, hi = _gb(1 << 24), _gb(2 << 24)

    def rc(factor, px, py, handle=None, rgb=1 << 20):
        prm = capi.UpscaleParams(**{"factor": factor, **capi.UPSCALE_DEFAULTS})
        return lib.rayz_hip_upscaler_run_phase(handle, C.byref(prm), px, py, C.c_void_p(rgb), None, C.byref(lo), C.byref(hi), C.c_void_p(2 << 20),
                                               None, None, None)

    for f in (2, 3, 4):
        for px in range(f):
            assert rc(f, px, f - 1 - px) == capi.ERR_STATE
        for px, py in ((f, 0), (0, f), (f, f), (1 << 31, 0)):
            assert rc(f, px, py) == capi.ERR_BAD_ARG and b"phase" in lib.rayz_hip_last_error(), (f, px, py)
    assert rc(5, 0, 0) == capi.ERR_BAD_ARG and b"factor" in lib.rayz_hip_last_error()
    assert rc(2, 1, 1, rgb=None) == capi.ERR_BAD_ARG
    assert "rayz_hip_upscaler_run_phase" in {p[0] for p in capi.PROTOTYPES}
