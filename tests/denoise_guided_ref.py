"""The CPU side of the guided denoiser's tests: builds tests/denoise_guided_mirror.cpp (the restatement of DESIGN.md §4.13) with
`g++ -O2 -ffp-contract=off`, as tests/denoise_ref.py builds the unguided mirror, and runs it on numpy arrays."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ALBEDO = 1  # RAYZ_DENOISE_ALBEDO
VCAP = np.float32(2.0 ** 32)

_lib = None
_F = C.POINTER(C.c_float)


def load():
    global _lib
    if _lib is not None:
        return _lib
    gxx = shutil.which("g++")
    if not gxx:
        raise RuntimeError("no g++: the guided denoiser's CPU mirror cannot be built")
    so = os.path.join(tempfile.mkdtemp(prefix="denoise_guided_mirror_"), "denoise_guided_mirror.so")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "denoise_guided_mirror.cpp")], check=True, capture_output=True, timeout=300)
    lib = C.CDLL(so)
    lib.denoise_guided_mirror_pack.argtypes = [_F, _F, C.POINTER(C.c_int32), _F, _F, _F, _F, _F, _F, _F, C.c_size_t]
    lib.denoise_guided_mirror_level.argtypes = [_F, _F, _F, _F, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float,
                                                C.c_float, C.c_uint32, C.c_uint32]
    lib.denoise_guided_mirror_finish.argtypes = [_F, _F, _F, _F, C.c_size_t]
    for f in (lib.denoise_guided_mirror_pack, lib.denoise_guided_mirror_level, lib.denoise_guided_mirror_finish):
        f.restype = None
    _lib = lib
    return lib


def _f(a):
    return a.ctypes.data_as(_F)


def denoise(rgb, var_rgb, index, normal, point, albedo=None, levels=5, normal_power_log2=6, flags=ALBEDO, sigma_color=2.0,
            sigma_plane=0.25, var_floor=1e-4, each_level=False, packed=False):
    """§4.13 on a (h, w, 3) float32 frame and its (h, w, 3) float32 per-channel variance.  Returns (rgb (h, w, 3), var (h, w)) — with
    `each_level` the list of those pairs for 1, 2, .., levels levels; with `packed` only the pack pass's v, (h, w)."""
    lib = load()
    h, w = index.shape
    n = h * w
    rgb, var_rgb, normal, point = (np.ascontiguousarray(a, dtype=np.float32).reshape(n, 3) for a in (rgb, var_rgb, normal, point))
    index = np.ascontiguousarray(index, dtype=np.int32).reshape(n)
    demod = bool(flags & ALBEDO)
    if demod:
        albedo = np.ascontiguousarray(albedo, dtype=np.float32).reshape(n, 3)
    ga, gb, mod, a, b = (np.empty((n, 4), np.float32) for _ in range(5))
    lib.denoise_guided_mirror_pack(_f(rgb), _f(var_rgb), index.ctypes.data_as(C.POINTER(C.c_int32)), _f(normal), _f(point),
                                   _f(albedo) if demod else None, _f(ga), _f(gb), _f(mod), _f(a), n)
    if packed:
        return a[:, 3].reshape(h, w).copy()
    with np.errstate(over="ignore"):
        sp2 = np.float32(sigma_plane) * np.float32(sigma_plane)
        sc2 = np.float32(sigma_color) * np.float32(sigma_color)
    outs = []
    for l in range(levels):
        lib.denoise_guided_mirror_level(_f(ga), _f(gb), _f(a), _f(b), w, h, l, normal_power_log2, float(sp2), float(sc2),
                                        float(np.float32(var_floor)), 0, h)
        a, b = b, a
        if each_level or l + 1 == levels:
            out, var = np.empty((n, 3), np.float32), np.empty(n, np.float32)
            lib.denoise_guided_mirror_finish(_f(a), _f(mod), _f(out), _f(var), n)
            outs.append((out.reshape(h, w, 3), var.reshape(h, w)))
    return outs if each_level else outs[-1]
