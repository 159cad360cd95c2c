"""The CPU side of the upscaler tests: builds tests/upscale_mirror.cpp (the restatement of DESIGN.md §4.20) with
`g++ -O2 -ffp-contract=off` and runs it on numpy arrays."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ALBEDO = 1  # RAYZ_DENOISE_ALBEDO
VCAP = np.float32(4294967296.0)
DEFAULTS = dict(normal_power_log2=6, flags=ALBEDO, sigma_plane=0.25)

_lib = None
_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)


def load():
    global _lib
    if _lib is not None:
        return _lib
    gxx = shutil.which("g++")
    if not gxx:
        raise RuntimeError("no g++: the upscaler's CPU mirror cannot be built")
    so = os.path.join(tempfile.mkdtemp(prefix="upscale_mirror_"), "upscale_mirror.so")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "upscale_mirror.cpp")],
                   check=True, capture_output=True, timeout=300)
    lib = C.CDLL(so)
    lib.upscale_mirror.argtypes = [_F, _F, _I, _F, _F, _F, _I, _F, _F, _F, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, _F, _F,
                                   C.POINTER(C.c_uint8)]
    lib.upscale_mirror.restype = None
    _lib = lib
    return lib


class Guides:
    """A G-buffer as numpy arrays: index (h, w) int32; normal, point, albedo (h, w, 3) float32."""

    def __init__(self, index, normal, point, albedo=None):
        self.index = np.ascontiguousarray(index, dtype=np.int32)
        self.normal = np.ascontiguousarray(normal, dtype=np.float32)
        self.point = np.ascontiguousarray(point, dtype=np.float32)
        self.albedo = None if albedo is None else np.ascontiguousarray(albedo, dtype=np.float32)


def upscale(rgb_lo, g_lo, g_hi, factor, var_rgb=None, normal_power_log2=6, flags=ALBEDO, sigma_plane=0.25):
    """§4.20: returns (out, var or None, stage): (H, W, 3) float32, the same or None without `var_rgb`, (H, W) uint8."""
    lib = load()
    h, w = g_lo.index.shape
    H, W = g_hi.index.shape
    assert (H, W) == (factor * h, factor * w), ((H, W), (h, w), factor)
    rgb_lo = np.ascontiguousarray(rgb_lo, dtype=np.float32)
    assert rgb_lo.shape == (h, w, 3)
    if var_rgb is not None:
        var_rgb = np.ascontiguousarray(var_rgb, dtype=np.float32)
        assert var_rgb.shape == (h, w, 3)
    demod = bool(flags & ALBEDO)
    f = lambda a: a.ctypes.data_as(_F)
    i = lambda a: a.ctypes.data_as(_I)
    with np.errstate(over="ignore"):
        sp2 = np.float32(sigma_plane) * np.float32(sigma_plane)
    out = np.empty((H, W, 3), np.float32)
    var = np.empty((H, W, 3), np.float32) if var_rgb is not None else None
    stage = np.empty((H, W), np.uint8)
    lib.upscale_mirror(f(rgb_lo), f(var_rgb) if var_rgb is not None else None, i(g_lo.index), f(g_lo.normal), f(g_lo.point),
                       f(g_lo.albedo) if demod else None, i(g_hi.index), f(g_hi.normal), f(g_hi.point), f(g_hi.albedo) if demod else None,
                       w, h, factor, normal_power_log2, float(sp2), f(out), f(var) if var is not None else None,
                       stage.ctypes.data_as(C.POINTER(C.c_uint8)))
    return out, var, stage
