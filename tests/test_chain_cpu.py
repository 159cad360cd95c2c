"""Specular-chain G-buffers (rayz_hip_scene_query_camera_chain) without a GPU: the refusals are made before any HIP
call, the contract's restatement (chain_ref.chain on the oracle backend) meets hand-derived exact cases, and the new kernels'
metadata as compiled for gfx950 — no vector register spilled, no scratch, beside unchanged counts of the existing kernels."""
import ctypes as C

import numpy as np
import pytest

import chain_ref
import isa_asm
from rayz_amd import capi, tracer

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
TMIN = 1e-3
M = chain_ref.KEY_MUL


def axial_camera():
    """Pixel (0, 0)'s centre lies on the axis: getRay(0, 0, null) = origin (0, 0, 0), direction (0, 0, -1) exactly."""
    return capi.CameraDesc(look_from=capi.D3(0, 0, 0), px_du=capi.D3(0.25, 0, 0), px_dv=capi.D3(0, -0.25, 0), px_origin=capi.D3(0, 0, -1),
                           defocus_u=capi.D3(0, 0, 0), defocus_v=capi.D3(0, 0, 0), defocus=0)


def scene(build):
    """A tracer whose pool `build(pool, white)` fills; the camera is not used."""
    t = tracer.Tracer.init(8, 40.0, 1.0, 0.0, (0, 0, 0), (0, 0, -1), (0, 1, 0), seed=1)
    build(t.pool, t.pool.add_solid_texture((0.5, 0.25, 0.75)))
    return t


def run(oracle, t, precision, max_depth, max_fuzz=0.25):
    be = chain_ref.OracleBackend(oracle, t.scene_desc(), precision)
    r = chain_ref.chain(be, axial_camera(), np.array([0]), np.array([0]), TMIN, max_depth, max_fuzz)
    return {k: v[0] for k, v in r.items()}


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_chain_arguments_are_refused_before_any_hip_call(built):
    """On a machine without a GPU a HIP call would fail with NO_DEVICE or ERR_HIP; these are BAD_ARG with their own message."""
    lib = capi.load()
    t = tracer.threeSpheres(32, seed=1)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    h = C.c_void_p()
    assert lib.rayz_hip_scene_create(C.byref(sd), C.byref(h)) == capi.OK
    try:
        out, co = capi.QueryOutputs(), capi.ChainOutputs()

        def call(chain, outputs=out, params=p, camera=cam, scene=h):
            return lib.rayz_hip_scene_query_camera_chain(scene, C.byref(camera) if camera else None, C.byref(params) if params else None,
                                                         C.byref(chain) if chain else None, C.byref(outputs) if outputs else None,
                                                         C.byref(co), None)

        assert call(capi.ChainParams(max_depth=capi.CHAIN_MAX_DEPTH + 1, max_fuzz=0.25)) == capi.ERR_BAD_ARG
        assert b"max_depth 17" in lib.rayz_hip_last_error()
        for bad in (float("nan"), -0.5, -float("inf")):
            assert call(capi.ChainParams(max_depth=4, max_fuzz=bad)) == capi.ERR_BAD_ARG, bad
            assert b"max_fuzz" in lib.rayz_hip_last_error()
        assert call(capi.ChainParams(max_depth=4, max_fuzz=0.25), outputs=None) == capi.ERR_BAD_ARG
        assert b"outputs is null" in lib.rayz_hip_last_error()
        assert call(None, outputs=None) == capi.ERR_BAD_ARG  # (NULL chain: the defaults, checked like any)
        # .. and what rayz_hip_scene_query_camera refuses
        assert call(None, params=None) == capi.ERR_BAD_ARG and call(None, camera=None) == capi.ERR_BAD_ARG
        assert call(None, scene=None) == capi.ERR_BAD_ARG
        q = capi.RenderParams.from_buffer_copy(p)
        q.shard_index, q.shard_count = 3, 2
        assert call(None, params=q) == capi.ERR_BAD_ARG and b"shard_index" in lib.rayz_hip_last_error()
        q = capi.RenderParams.from_buffer_copy(p)
        q.tmin = float("nan")
        assert call(None, params=q) == capi.ERR_BAD_ARG
        assert capi.CHAIN_DEFAULTS == {"max_depth": 4, "max_fuzz": 0.25} and capi.CHAIN_MAX_DEPTH == 16
    finally:
        lib.rayz_hip_scene_destroy(h)


def test_denoiser_keys_need_a_handle(built):
    lib = capi.load()
    assert lib.rayz_hip_denoiser_set_keys(None, None) == capi.ERR_STATE and b"denoiser" in lib.rayz_hip_last_error()


# ---- hand-derived exact cases of the contract ----------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", [F32, F64])
def test_axial_ray_onto_a_mirror_returns_and_misses(oracle, precision):
    """n = (0, 0, 1) at (0, 0, -4): reflect((0, 0, -1), n) = (0, 0, 1), back through the origin into nothing."""
    t = scene(lambda P, tex: P.add_sphere((0, 0, -5), 1.0, P.add_metallic(tex, 0.0)))
    r = run(oracle, t, precision, 4)
    assert (r["index"], r["depth"], r["first_index"], r["key"], r["segments"]) == (-1, 1, 0, 1, 2)
    assert r["t"] == np.inf and r["material"] == -1 and not r["albedo"].any() and not r["point"].any()
    assert r["dir"].tolist() == [0.0, 0.0, 1.0]
    # max_depth 0 is the first hit
    r = run(oracle, t, precision, 0)
    assert (r["index"], r["depth"], r["first_index"], r["key"]) == (0, 0, 0, 0)
    assert r["point"].tolist() == [0.0, 0.0, -4.0] and r["normal"].tolist() == [0.0, 0.0, 1.0] and r["front_face"] == 1
    assert r["specular_end"]


@pytest.mark.parametrize("precision", [F32, F64])
def test_axial_ray_through_a_glass_ball_onto_a_diffuse_sphere(oracle, precision):
    """Normal incidence: cos = 1, the tangential part of the refraction is exactly 0 on the way in and on the way out."""
    def build(P, tex):
        P.add_sphere((0, 0, -5), 1.0, P.add_dielectric(1.5))
        P.add_sphere((0, 0, -10), 1.0, P.add_diffuse(tex))

    r = run(oracle, scene(build), precision, 4)
    assert (r["index"], r["depth"], r["first_index"], r["segments"]) == (1, 2, 0, 3)
    assert r["key"] == (1 * M + 1) & 0xFFFFFFFF
    assert r["dir"].tolist() == [0.0, 0.0, -1.0]  # undeviated, exactly
    assert r["point"].tolist() == [0.0, 0.0, -9.0] and r["normal"].tolist() == [0.0, 0.0, 1.0] and r["front_face"] == 1
    assert r["t"] == 3.0  # from the far side of the ball, (0, 0, -6)
    want = np.array([0.5, 0.25, 0.75])  # the diffuse texture; glass tints by (1, 1, 1)
    assert r["albedo"].tolist() == want.tolist() and not r["tir"]


@pytest.mark.parametrize("precision", [F32, F64])
def test_two_facing_mirrors_end_at_max_depth_on_a_specular_record(oracle, precision):
    def build(P, tex):
        m = P.add_metallic(tex, 0.0)
        P.add_sphere((0, 0, -5), 1.0, m)
        P.add_sphere((0, 0, 5), 1.0, m)

    t = scene(build)
    for depth in (1, 4, 16):
        r = run(oracle, t, precision, depth)
        assert r["depth"] == depth and r["segments"] == depth + 1 and r["specular_end"]
        assert r["index"] == depth % 2 and r["first_index"] == 0  # 0, 1, 0, 1, ..
        key = 0
        for s in range(depth):
            key = (key * M + (s % 2) + 1) & 0xFFFFFFFF
        assert r["key"] == key
        assert r["point"].tolist() == [0.0, 0.0, -4.0 if depth % 2 == 0 else 4.0]
        a = np.array([0.5, 0.25, 0.75]).astype(np.float32 if precision == F32 else np.float64)
        want = np.ones(3, a.dtype)
        for s in range(depth + 1):  # the tint of `depth` mirrors, then the record's own albedo
            want = want * a
        assert r["albedo"].tolist() == want.astype(np.float64).tolist()


@pytest.mark.parametrize("precision", [F32, F64])
def test_max_fuzz_decides_whether_a_rough_metal_is_followed(oracle, precision):
    t = scene(lambda P, tex: P.add_sphere((0, 0, -5), 1.0, P.add_metallic(tex, 0.6)))
    r = run(oracle, t, precision, 4, max_fuzz=0.25)
    assert (r["index"], r["depth"], r["key"], r["first_index"]) == (0, 0, 0, 0) and r["fuzz_stop"] and not r["specular_end"]
    assert r["albedo"].tolist() == [0.5, 0.25, 0.75]
    r = run(oracle, t, precision, 4, max_fuzz=1.0)  # followed, along the PURE mirror direction: no fuzz, no draw
    assert (r["index"], r["depth"], r["key"], r["first_index"]) == (-1, 1, 1, 0) and not r["fuzz_stop"]
    assert r["dir"].tolist() == [0.0, 0.0, 1.0]


# ---- the compiled kernels ------------------------------------------------------------------------------------------------------
def test_chain_kernels_codegen_and_the_existing_kernel_counts():
    meta = isa_asm.metadata(isa_asm.device_asm())
    chain = {k: v for k, v in meta.items() if "chain_kernel" in k}
    # flat f32 / f64, BVH f32 / f64 x two node-record formats
    assert len(chain) == 6 and sum("chain_kernel_bvh" in k for k in chain) == 4, sorted(chain)
    # .. and the one-workgroup launch that hands them their output pointers
    new = {k: v for k, v in meta.items() if "chain" in k}
    assert set(new) - set(chain) == {k for k in new if "chain_outputs_kernel" in k} and len(new) == 7, sorted(new)
    for name, f in new.items():
        assert not any(s in name for s in ("query", "trace_kernel", "adaptive_pass_kernel", "denoise_")), name
        assert int(f["vgpr_spill_count"]) == 0, (name, f["vgpr_spill_count"])
        assert int(f["private_segment_fixed_size"]) == 0, (name, f["private_segment_fixed_size"])
    # the existing kernels are all still there, and no more of them
    assert sum("query" in k for k in meta) == 8, sorted(k for k in meta if "query" in k)
    assert sum("trace_kernel" in k for k in meta) == 6
    assert sum("denoise_" in k for k in meta) == 18


# ---- the GPU test's scene shows what that test asserts (checked here, where no GPU is needed) ------------------------------------
def test_the_gpu_tests_frames_show_every_case(oracle):
    import chain_scenes as cs

    px, py = cs.shape_pixels(cs.W, cs.H)
    for precision in (F32, F64):
        be = {}
        for cam in cs.CAMERAS:
            t = cs.build(cam)
            be[cam] = (t, chain_ref.OracleBackend(oracle, t.scene_desc(), precision))
        for max_depth in sorted(cs.DEPTHS, reverse=True):
            n, first = {}, set()
            for cam, (t, b) in be.items():
                r = chain_ref.chain(b, t.camera_desc(), px, py, cs.TMIN, max_depth, cs.MAX_FUZZ)
                for k, v in cs.classes(r, max_depth).items():
                    n[k] = n.get(k, 0) + v
                first |= set(r["first_index"].tolist())
                assert (r["segments"] == r["depth"] + 1).all() and r["depth"].max() <= max_depth
            need = ["at max_depth on a specular record", "stopped by max_fuzz"] + (["a miss after a followed hit", "total internal reflection"]
                                                                                   if max_depth >= 1 else []) + (["depth >= 2"] if max_depth >= 2 else [])
            for k in need:
                assert n[k] >= 16, (precision, max_depth, k, n)
            assert {-1, 0, 1, 2, 3, 4, 5, 8, 9, 10, 11} <= first  # sky, ground, every sphere a camera ray can reach first, the triangles
