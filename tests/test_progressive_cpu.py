"""The progressive entry points (rayz_hip_progressive_*) without a GPU: they are exported and bound, refuse null handles
and pointers, validate their arguments as rayz_hip_render_device does, and fail without a device instead of computing."""
import ctypes as C

import pytest

from rayz_amd import capi, render, tracer

NAMES = ["rayz_hip_progressive_create", "rayz_hip_progressive_step", "rayz_hip_progressive_step_f64",
         "rayz_hip_progressive_info", "rayz_hip_progressive_destroy"]


def _scene(lib, t):
    h = C.c_void_p()
    assert lib.rayz_hip_scene_create(C.byref(t.scene_desc()), C.byref(h)) == capi.OK
    return h


def test_progressive_symbols_are_exported_and_bound(built):
    lib = capi.load()
    bound = {p[0] for p in capi.PROTOTYPES}
    for n in NAMES:
        assert hasattr(lib, n) and n in bound, n
    assert hasattr(render.DeviceScene, "progressive") and hasattr(render, "Progressive")


def test_null_handles_and_pointers(built):
    lib = capi.load()
    t = tracer.threeSpheres(32, seed=1)
    cam, p = t.camera_desc(), t.params()
    out = C.c_void_p()
    assert lib.rayz_hip_progressive_create(None, C.byref(cam), C.byref(p), C.byref(out)) == capi.ERR_STATE
    assert out.value is None
    s = _scene(lib, t)
    try:
        assert lib.rayz_hip_progressive_create(s, None, C.byref(p), C.byref(out)) == capi.ERR_BAD_ARG
        assert lib.rayz_hip_progressive_create(s, C.byref(cam), None, C.byref(out)) == capi.ERR_BAD_ARG
        assert lib.rayz_hip_progressive_create(s, C.byref(cam), C.byref(p), None) == capi.ERR_BAD_ARG
    finally:
        lib.rayz_hip_scene_destroy(s)
    assert lib.rayz_hip_progressive_step(None, 0, None, None) == capi.ERR_STATE
    assert lib.rayz_hip_progressive_step_f64(None, 0, None, None) == capi.ERR_STATE
    n = C.c_uint32()
    assert lib.rayz_hip_progressive_info(None, C.byref(n), None, None, None) == capi.ERR_STATE
    assert b"null" in lib.rayz_hip_last_error()
    assert lib.rayz_hip_progressive_destroy(None) == capi.OK


def test_create_without_a_device_is_an_error_not_a_fallback(built):
    import torch

    if torch.cuda.is_available():
        pytest.skip("a GPU is present; covered by the gpu tests")
    lib = capi.load()
    assert lib.rayz_hip_init(0) == capi.ERR_NO_DEVICE
    t = tracer.threeSpheres(32, seed=1)
    s = _scene(lib, t)
    out = C.c_void_p()
    try:
        rc = lib.rayz_hip_progressive_create(s, C.byref(t.camera_desc()), C.byref(t.params()), C.byref(out))
        assert rc == capi.ERR_NO_DEVICE and out.value is None
    finally:
        lib.rayz_hip_scene_destroy(s)
    with pytest.raises(capi.RayzHipError):
        render.DeviceScene(t.scene_desc()).progressive(t.camera_desc(), t.params())


@pytest.mark.parametrize("field,value,msg", [("samples_per_px", 0, b"samples_per_px"), ("width", 0, b"width"),
                                             ("precision", 9, b"precision"), ("traversal", 7, b"traversal"),
                                             ("shard_index", 3, b"shard_index"), ("tmin", float("nan"), b"NaN")])
def test_create_refuses_what_render_refuses(built, field, value, msg):
    """check_render_args runs before anything else: the refusal is the render entry's, with or without a device."""
    lib = capi.load()
    t = tracer.threeSpheres(32, seed=1)
    p = t.params()
    setattr(p, field, value)
    if field == "shard_index":
        p.shard_count = 2
    s = _scene(lib, t)
    out = C.c_void_p()
    try:
        rc = lib.rayz_hip_progressive_create(s, C.byref(t.camera_desc()), C.byref(p), C.byref(out))
        assert rc == capi.ERR_BAD_ARG and msg in lib.rayz_hip_last_error(), (rc, lib.rayz_hip_last_error())
        assert out.value is None
        assert lib.rayz_hip_render_device(s, C.byref(t.camera_desc()), C.byref(p), None, None) == capi.ERR_BAD_ARG
    finally:
        lib.rayz_hip_scene_destroy(s)


def test_create_refuses_too_many_chunks(built):
    lib = capi.load()
    t = tracer.threeSpheres(32, seed=1)
    p = capi.RenderParams(width=4, height=4, samples_per_px=1 << 30, chunk_spp=1)
    s = _scene(lib, t)
    out = C.c_void_p()
    try:
        rc = lib.rayz_hip_progressive_create(s, C.byref(t.camera_desc()), C.byref(p), C.byref(out))
        assert rc == capi.ERR_BAD_ARG and b"chunks per pixel" in lib.rayz_hip_last_error()
    finally:
        lib.rayz_hip_scene_destroy(s)
