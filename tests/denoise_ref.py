"""The CPU side of the denoiser tests: builds tests/denoise_mirror.cpp (the restatement of DESIGN.md §4.11) with
`g++ -O2 -ffp-contract=off` and runs it on numpy arrays.  ctypes releases the GIL, so the rows of a level are dealt to a few
threads: every pixel of a level depends on the previous level only, the result does not depend on the split."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ALBEDO = 1  # RAYZ_DENOISE_ALBEDO
DEFAULTS = dict(levels=5, normal_power_log2=6, flags=ALBEDO, sigma_color=0.5, sigma_plane=0.25)

_lib = None
_F = C.POINTER(C.c_float)


def load():
    global _lib
    if _lib is not None:
        return _lib
    gxx = shutil.which("g++")
    if not gxx:
        raise RuntimeError("no g++: the denoiser's CPU mirror cannot be built")
    so = os.path.join(tempfile.mkdtemp(prefix="denoise_mirror_"), "denoise_mirror.so")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "denoise_mirror.cpp")],
                   check=True, capture_output=True, timeout=300)
    lib = C.CDLL(so)
    lib.denoise_mirror_pack.argtypes = [_F, C.POINTER(C.c_int32), _F, _F, _F, _F, _F, _F, _F, C.c_size_t]
    lib.denoise_mirror_level.argtypes = [_F, _F, _F, _F, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_float,
                                         C.c_uint32, C.c_uint32]
    lib.denoise_mirror_finish.argtypes = [_F, _F, _F, C.c_size_t]
    for f in (lib.denoise_mirror_pack, lib.denoise_mirror_level, lib.denoise_mirror_finish):
        f.restype = None
    _lib = lib
    return lib


def _f(a):
    return a.ctypes.data_as(_F)


def denoise(rgb, index, normal, point, albedo=None, levels=5, normal_power_log2=6, flags=ALBEDO, sigma_color=0.5, sigma_plane=0.25,
            threads=16, each_level=False):
    """§4.11 on a (h, w, 3) float32 frame with (h, w) int32 index and (h, w, 3) float32 normal / point / albedo.  Returns (h, w, 3);
    `each_level`: the list of the results for 1, 2, .., levels levels (a run of L levels is a run of L + 1 stopped one level early and
    re-modulated there)."""
    lib = load()
    h, w = index.shape
    n = h * w
    rgb, normal, point = (np.ascontiguousarray(a, dtype=np.float32).reshape(n, 3) for a in (rgb, normal, point))
    index = np.ascontiguousarray(index, dtype=np.int32).reshape(n)
    demod = bool(flags & ALBEDO)
    if demod:
        albedo = np.ascontiguousarray(albedo, dtype=np.float32).reshape(n, 3)
    ga, gb, mod, a, b = (np.empty((n, 4), np.float32) for _ in range(5))
    lib.denoise_mirror_pack(_f(rgb), index.ctypes.data_as(C.POINTER(C.c_int32)), _f(normal), _f(point), _f(albedo) if demod else None,
                            _f(ga), _f(gb), _f(mod), _f(a), n)
    with np.errstate(over="ignore"):
        sp2 = np.float32(sigma_plane) * np.float32(sigma_plane)
        sc2 = np.float32(sigma_color) * np.float32(sigma_color)
    levels = levels or 5
    threads = max(1, min(threads, h // 16 or 1))
    cuts = [h * t // threads for t in range(threads + 1)]
    outs = []
    with ThreadPoolExecutor(threads) as pool:
        for l in range(levels):
            jobs = [pool.submit(lib.denoise_mirror_level, _f(ga), _f(gb), _f(a), _f(b), w, h, l, normal_power_log2, float(sp2), float(sc2),
                                cuts[t], cuts[t + 1]) for t in range(threads)]
            for j in jobs:
                j.result()
            a, b = b, a
            if each_level or l + 1 == levels:
                out = np.empty((n, 3), np.float32)
                lib.denoise_mirror_finish(_f(a), _f(mod), _f(out), n)
                outs.append(out.reshape(h, w, 3))
    return outs if each_level else outs[-1]
