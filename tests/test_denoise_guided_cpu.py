"""The variance-guided denoiser without a GPU: the CPU restatement (tests/denoise_guided_mirror.cpp) against the
hand-derived exact answers of tests/denoise_guided_cases.py; what the pack pass makes of a NaN, an infinite and a negative variance;
the restatement against the unguided one where the two must agree; and the binding — struct layout, prototypes, every
RAYZ_ERR_BAD_ARG path of rayz_hip_denoiser_run_guided (all checked before the handle, so none needs a device), the ABI version."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import denoise_guided_cases as cases
import denoise_guided_ref
import denoise_ref
from denoise_cases import synthetic
from denoise_guided_cases import guided_variance
from rayz_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def run_mirror(c, **over):
    return denoise_guided_ref.denoise(c.rgb, c.var_rgb, c.index, c.normal, c.point, c.albedo, **{**c.params, **over})


@pytest.mark.parametrize("case", cases.cases(), ids=lambda c: c.name)
def test_mirror_gives_the_hand_derived_answers(case):
    """exact() reproduces the docstring's closed forms at the hand pixels, and the mirror equals exact()'s rationals, rounded once,
    bit for bit at every pixel exact() knows."""
    known = cases.exact(case)
    for p, (col, var) in case.hand.items():
        assert p in known, (case.name, p)
        assert list(known[p][0]) == list(col) and known[p][1] == var, (case.name, p, known[p], (col, var))
    rgb, var = run_mirror(case)
    case.check(rgb, var, "mirror")
    assert np.isfinite(rgb[case.index >= 0]).all() and np.isfinite(var[case.index >= 0]).all()


def test_hand_values_are_the_ones_the_contract_names():
    """The figures DESIGN.md §4.13 quotes: an interior pixel of a uniform field keeps 1225/16384 of its variance per level."""
    one, two = cases.uniform(1), cases.uniform(2)
    assert one.hand[(3, 3)][1] == cases.F(1, 2) * cases.F(1225, 16384)
    assert two.hand[(6, 6)][1] == cases.F(1, 2) * cases.F(1225, 16384) ** 2
    rgb, var = run_mirror(one)
    assert var[3, 3] == np.float32(0.5 * 1225 / 16384) and np.array_equal(rgb[3, 3], one.rgb[3, 3])
    assert var[0, 0] == cases.round_f32(cases.F(1, 2) * cases.F(2809, 14641))
    _, var = run_mirror(two)
    assert var[6, 6] == np.float32(0.5 * (1225 / 16384) ** 2)


def test_the_step_weights_are_the_derived_rationals():
    """v = 0 with the floor: the cross-edge weight is 1/4; v = VCAP: it is 1, the plain B-spline."""
    rgb, var = run_mirror(cases.step_v0())
    assert rgb[2, 2, 0] == cases.round_f32(cases.F(5, 49)) and rgb[2, 3, 0] == cases.round_f32(cases.F(8, 9)) and (var == 0).all()
    rgb, var = run_mirror(cases.step_vcap())
    assert rgb[2, 2, 0] == np.float32(5 / 16) and rgb[2, 3, 0] == cases.round_f32(cases.F(2, 3))
    assert var[2, 2] == np.float32(1225 * 2.0 ** 18)
    # .. and 1 to the last bit means: the same bits as the colour term switched off
    off, _ = run_mirror(cases.step_vcap(), sigma_color=INF)
    assert np.array_equal(rgb.view(np.uint32), off.view(np.uint32))


@pytest.mark.parametrize("label,case,pixel,v", cases.odd_variances(), ids=lambda x: x if isinstance(x, str) else "")
def test_a_nan_an_infinite_and_a_negative_variance(label, case, pixel, v):
    packed = denoise_guided_ref.denoise(case.rgb, case.var_rgb, case.index, case.normal, case.point, None, **case.params, packed=True)
    assert packed[pixel] == np.float32(float(v)), (label, packed[pixel])
    assert cases.pack_v(case)[pixel] == v
    others = np.ones(packed.shape, bool)
    others[pixel] = False
    assert (packed[others] == np.float32(0.5)).all()
    for levels in (1, 2, 5):
        rgb, var = run_mirror(case, levels=levels)
        assert np.isfinite(rgb).all() and np.isfinite(var).all() and (var >= 0).all(), (label, levels)


def test_the_prefilter_skips_a_background_pixel():
    case = cases.background_neighbour()
    rgb, var = run_mirror(case)
    assert rgb[1, 1, 0] == cases.round_f32(cases.F(3, 77)) and var[1, 1] == cases.round_f32(cases.F(877, 11858))
    assert np.isfinite(rgb[case.index >= 0]).all()


@pytest.mark.parametrize("w,h", [(1, 1), (5, 3), (33, 9), (45, 23)])
def test_with_the_colour_term_off_the_colour_is_the_unguided_filters(w, h):
    """sigma_color = +inf makes wc = 1 in both filters, and everything else of a tap is §4.11's in both: the guided mirror's COLOUR
    equals the unguided mirror's bit for bit, for any variance (NaN and +inf included) — two restatements written apart agree."""
    rgb, index, normal, point, albedo = synthetic(w, h, 31 * w + h)
    var = guided_variance(rgb, 7)
    for flags in (1, 0):
        a = denoise_ref.denoise(rgb, index, normal, point, albedo, levels=5, flags=flags, sigma_color=INF, each_level=True)
        b = denoise_guided_ref.denoise(rgb, var, index, normal, point, albedo, levels=5, flags=flags, sigma_color=INF, each_level=True)
        for l in range(5):
            assert np.array_equal(a[l].view(np.uint32), b[l][0].view(np.uint32)), (w, h, flags, l)


def test_a_finite_sigma_changes_the_image_and_stays_finite():
    """On the synthetic guides with every odd variance value: finite output on every hit and background pixel, and the colour term
    does something (the image differs from the colour-term-off one)."""
    rgb, index, normal, point, albedo = synthetic(45, 23, 4523)
    var = guided_variance(rgb, 3)
    a, va = denoise_guided_ref.denoise(rgb, var, index, normal, point, albedo, levels=3, sigma_color=2.0, var_floor=1e-4)
    b, _ = denoise_guided_ref.denoise(rgb, var, index, normal, point, albedo, levels=3, sigma_color=INF)
    assert np.isfinite(a).all() and np.isfinite(va).all() and (va >= 0).all()
    assert not np.array_equal(a, b)


# ---- the binding --------------------------------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayz_hip.h")).read(), flags=re.S)


C_TYPES = {"uint32_t": (C.c_uint32, "u32"), "double": (C.c_double, "f64")}


def test_struct_layout_matches_the_header_and_the_zig_text(built):
    m = re.search(r"typedef struct RayzDenoiseGuidedParams \{(.*?)\} RayzDenoiseGuidedParams;", _header(), flags=re.S)
    fields = []
    for decl in m.group(1).split(";"):
        for name in (decl.split()[1:] if decl.split() else []):
            fields.append((decl.split()[0], name.rstrip(",")))
    assert [n for _, n in fields] == ["levels", "normal_power_log2", "flags", "_pad", "sigma_color", "sigma_plane", "var_floor"]
    assert [(n, C_TYPES[t][0]) for t, n in fields] == list(capi.DenoiseGuidedParams._fields_)
    off = {n: getattr(capi.DenoiseGuidedParams, n).offset for _, n in fields}
    assert off == {"levels": 0, "normal_power_log2": 4, "flags": 8, "_pad": 12, "sigma_color": 16, "sigma_plane": 24, "var_floor": 32}
    assert C.sizeof(capi.DenoiseGuidedParams) == 40
    # RayzDenoiseParams is a prefix of it and unchanged
    assert list(capi.DenoiseGuidedParams._fields_)[:6] == list(capi.DenoiseParams._fields_) and C.sizeof(capi.DenoiseParams) == 32
    zig = open(os.path.join(ROOT, "rayz_amd", "zig", "renderer_hip.zig")).read()
    z = re.search(r"pub const RayzDenoiseGuidedParams: type = extern struct \{(.*?)\n\};", zig, flags=re.S)
    zf = re.findall(r"^\s*(\w+): (\w+)", z.group(1), flags=re.M)
    assert zf == [(n, C_TYPES[t][1]) for t, n in fields]
    # the defaults the three layers state are one set
    hdr = _header()
    d = capi.DENOISE_GUIDED_DEFAULTS
    assert float(re.search(r"RAYZ_DENOISE_GUIDED_DEFAULT_SIGMA_COLOR (\S+)", hdr).group(1)) == d["sigma_color"]
    assert float(re.search(r"RAYZ_DENOISE_GUIDED_DEFAULT_VAR_FLOOR (\S+)", hdr).group(1)) == d["var_floor"]
    assert int(re.search(r"RAYZ_DENOISE_GUIDED_DEFAULT_LEVELS (\d+)u", hdr).group(1)) == d["levels"]
    assert float(re.search(r"sigma_color: f64 = ([^,]+),", z.group(1)).group(1)) == d["sigma_color"]
    assert float(re.search(r"var_floor: f64 = ([^,]+),", z.group(1)).group(1)) == d["var_floor"]


def test_prototypes_in_header_binding_and_zig(built):
    hdr = " ".join(_header().split())
    assert ("int rayz_hip_denoiser_run_guided(RayzDenoiser* dn, const RayzDenoiseGuidedParams* params, const float* d_rgb_in, "
            "const float* d_var_rgb, const RayzQueryOutputs* gbuffer, float* d_rgb_out, float* d_var_out_or_null, void* hip_stream);") in hdr
    assert "int rayz_hip_progressive_noise_rgb(RayzProgressive* pr, float* d_var_rgb, void* hip_stream);" in hdr
    protos = {p[0]: p for p in capi.PROTOTYPES}
    assert len(protos["rayz_hip_denoiser_run_guided"][2]) == 8 and len(protos["rayz_hip_progressive_noise_rgb"][2]) == 3
    lib = capi.load()
    assert hasattr(lib, "rayz_hip_denoiser_run_guided") and hasattr(lib, "rayz_hip_progressive_noise_rgb")
    zig = " ".join(open(os.path.join(ROOT, "rayz_amd", "zig", "renderer_hip.zig")).read().split())
    assert ("pub extern fn rayz_hip_denoiser_run_guided( dn: *RayzDenoiser, params: ?*const RayzDenoiseGuidedParams, d_rgb_in: [*]const f32, "
            "d_var_rgb: [*]const f32, gbuffer: *const RayzQueryOutputs, d_rgb_out: [*]f32, d_var_out: ?[*]f32, hip_stream: ?*anyopaque, ) c_int;") in zig
    assert "pub extern fn rayz_hip_progressive_noise_rgb(pr: *RayzProgressive, d_var_rgb: [*]f32, hip_stream: ?*anyopaque) c_int;" in zig


def test_abi_version_is_still_5(built):
    assert capi.load().rayz_hip_abi_version() == capi.ABI_VERSION == 5


def test_every_bad_argument_is_refused_before_the_handle(built):
    """All arguments are checked before the handle and nothing touches a device: with valid arguments and a null handle the answer is
    RAYZ_ERR_STATE, with any one bad argument RAYZ_ERR_BAD_ARG and a message that names it."""
    lib = capi.load()
    buf = C.c_void_p(4096)  # never dereferenced: the handle is refused first
    g = capi.QueryOutputs(index=4096, normal=4096, point=4096, albedo=4096)

    def run(prm=None, rgb=buf, var=buf, gb=g, out=buf, **over):
        p = capi.DenoiseGuidedParams(**{**capi.DENOISE_GUIDED_DEFAULTS, **over}) if prm is None else prm
        return lib.rayz_hip_denoiser_run_guided(None, C.byref(p) if p is not False else None, rgb, var, C.byref(gb) if gb is not None else None,
                                                out, None, None)

    assert run() == capi.ERR_STATE and b"not a denoiser handle" in lib.rayz_hip_last_error()
    assert run(prm=False) == capi.ERR_STATE  # NULL params: the defaults pass the checks
    assert run(sigma_color=INF) == capi.ERR_STATE and run(var_floor=INF) == capi.ERR_STATE and run(levels=0) == capi.ERR_STATE
    bad = [(dict(levels=9), b"levels"), (dict(normal_power_log2=17), b"normal_power_log2"), (dict(flags=2), b"flag"),
           (dict(sigma_color=0.0), b"sigma_color"), (dict(sigma_color=-1.0), b"sigma_color"), (dict(sigma_color=float("nan")), b"sigma_color"),
           (dict(sigma_color=1e-30), b"sigma_color"),  # its f32 square is 0
           (dict(sigma_plane=0.0), b"sigma_plane"), (dict(sigma_plane=float("nan")), b"sigma_plane"),
           (dict(var_floor=0.0), b"var_floor"), (dict(var_floor=-1e-4), b"var_floor"), (dict(var_floor=float("nan")), b"var_floor"),
           (dict(var_floor=1e-60), b"var_floor"),  # f32(var_floor) is 0
           (dict(sigma_color=1e-15, var_floor=1e-20), b"var_floor")]  # sc2 = 1e-30 and vf are positive, their f32 product is 0
    for over, word in bad:
        assert run(**over) == capi.ERR_BAD_ARG, over
        assert word in lib.rayz_hip_last_error(), (over, lib.rayz_hip_last_error())
    assert run(var=None) == capi.ERR_BAD_ARG and b"variance" in lib.rayz_hip_last_error()
    assert run(rgb=None) == capi.ERR_BAD_ARG and run(out=None) == capi.ERR_BAD_ARG and run(gb=None) == capi.ERR_BAD_ARG
    assert run(gb=capi.QueryOutputs(index=4096, normal=4096, point=4096)) == capi.ERR_BAD_ARG and b"albedo" in lib.rayz_hip_last_error()
    assert run(gb=capi.QueryOutputs(index=4096, normal=4096, point=4096), flags=0) == capi.ERR_STATE
    assert run(gb=capi.QueryOutputs(index=4096, normal=4096, albedo=4096)) == capi.ERR_BAD_ARG
    # the per-channel variance of a handle that is none
    assert lib.rayz_hip_progressive_noise_rgb(None, buf, None) == capi.ERR_STATE
