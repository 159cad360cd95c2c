"""The CPU side of the footprint-albedo tests: builds tests/footprint_mirror.cpp (the restatement of DESIGN.md §4.24) with
`g++ -O2 -ffp-contract=off` and runs it on numpy arrays."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))

_lib = None
_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)
_B = C.POINTER(C.c_uint8)


def load():
    global _lib
    if _lib is not None:
        return _lib
    gxx = shutil.which("g++")
    if not gxx:
        raise RuntimeError("no g++: the footprint albedo's CPU mirror cannot be built")
    so = os.path.join(tempfile.mkdtemp(prefix="footprint_mirror_"), "footprint_mirror.so")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "footprint_mirror.cpp")],
                   check=True, capture_output=True, timeout=300)
    lib = C.CDLL(so)
    lib.footprint_mirror.argtypes = [_I, _F, _I, _F, C.c_uint32, C.c_uint32, C.c_uint32, _F, _B]
    lib.footprint_mirror.restype = None
    _lib = lib
    return lib


def footprint(index_lo, albedo_lo, index_hi, albedo_hi, factor):
    """§4.24: returns (albedo (h, w, 3) float32, count (h, w) uint8).  The inputs are not modified."""
    lib = load()
    index_lo = np.ascontiguousarray(index_lo, dtype=np.int32)
    index_hi = np.ascontiguousarray(index_hi, dtype=np.int32)
    albedo_lo = np.ascontiguousarray(albedo_lo, dtype=np.float32)
    albedo_hi = np.ascontiguousarray(albedo_hi, dtype=np.float32)
    h, w = index_lo.shape
    assert index_hi.shape == (factor * h, factor * w), (index_hi.shape, (h, w), factor)
    assert albedo_lo.shape == (h, w, 3) and albedo_hi.shape == (factor * h, factor * w, 3)
    out = np.empty((h, w, 3), np.float32)
    count = np.empty((h, w), np.uint8)
    lib.footprint_mirror(index_lo.ctypes.data_as(_I), albedo_lo.ctypes.data_as(_F), index_hi.ctypes.data_as(_I), albedo_hi.ctypes.data_as(_F),
                         w, h, factor, out.ctypes.data_as(_F), count.ctypes.data_as(_B))
    return out, count


def footprint_guides(g_lo, g_hi, factor):
    """The same on two G-buffers (anything with .index and .albedo)."""
    return footprint(g_lo.index, g_lo.albedo, g_hi.index, g_hi.albedo, factor)
