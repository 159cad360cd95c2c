"""The CPU side of the tests of temporal accumulation's moments mode: builds tests/temporal_moments_mirror.cpp (the restatement
of DESIGN.md §4.16) with `g++ -O2 -ffp-contract=off`, as tests/temporal_ref.py builds its mirror, and runs it on numpy arrays.
`TemporalMoments` is the handle's state machine around it: two history buffers of five records, the previous camera (its matrix
from tests/temporal_ref.py: the host part of a step is §4.15's), the "has history" flag."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import temporal_ref
from temporal_ref import camera_key, camera_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULTS = dict(temporal_ref.DEFAULTS)
MOMENTS_DEFAULTS = {"w2_max": 0.25, "min_taps": 4.0}  # RAYZ_TEMPORAL_MOMENTS_DEFAULT_*
VCAP = temporal_ref.VCAP

_lib = None
_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)


def load():
    global _lib
    if _lib is not None:
        return _lib
    gxx = shutil.which("g++")
    if not gxx:
        raise RuntimeError("no g++: the moments mode's CPU mirror cannot be built")
    so = os.path.join(tempfile.mkdtemp(prefix="temporal_moments_mirror_"), "temporal_moments_mirror.so")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "temporal_moments_mirror.cpp")], check=True, capture_output=True, timeout=300)
    lib = C.CDLL(so)
    lib.temporal_moments_mirror_step.argtypes = [_F, _I, _F, _F] + [_F] * 9 + [_F, _F, _F, _F, C.c_uint32, C.c_uint32, C.c_int, C.c_int, _F, _F] + \
        [C.c_float] * 7
    lib.temporal_moments_mirror_step.restype = None
    _lib = lib
    return lib


def _f(a):
    return a.ctypes.data_as(_F)


class TemporalMoments:
    """The mirror's handle in moments mode: `step` is rayz_hip_temporal_step_moments on numpy arrays and returns (colour, variance,
    length, W2); `reset` is rayz_hip_temporal_reset.  `state()` returns the history the last step left: (c, v, g, p, m), each
    (h, w, 4) float32, the index as bits in g[..., 3], m = {m2, W2}."""

    def __init__(self, width, height):
        self.width, self.height = width, height
        n = width * height
        self.hist = [[np.zeros((n, 4), np.float32) for _ in range(5)] for _ in range(2)]
        self.cur = 0
        self.has_history = False
        self.key = None
        self.M, self.fr = np.zeros(9, np.float32), np.zeros(3, np.float32)
        self.last_static = None

    def reset(self):
        self.has_history = False

    def state(self):
        h, w = self.height, self.width
        return tuple(a.reshape(h, w, 4).copy() for a in self.hist[self.cur])

    def step(self, rgb, index, normal, point, camera, spp, **params):
        lib = load()
        unknown = set(params) - set(DEFAULTS) - set(MOMENTS_DEFAULTS)
        assert not unknown, unknown
        prm = {**DEFAULTS, **MOMENTS_DEFAULTS, **params}
        h, w = self.height, self.width
        n = h * w
        mf = camera_matrix(camera)
        if mf is None:
            raise ValueError("camera: det is 0 or not finite")
        rgb, normal, point = (np.ascontiguousarray(a, dtype=np.float32).reshape(n, 3) for a in (rgb, normal, point))
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(n)
        key = camera_key(camera)
        static = self.has_history and key == self.key
        (pc, _, pg, pp, pm), nxt = self.hist[self.cur], self.hist[self.cur ^ 1]
        out, vout = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        lout, wout = np.empty(n, np.float32), np.empty(n, np.float32)
        with np.errstate(over="ignore"):
            r = np.float32(prm["max_rel_dist"])
            r2 = r * r
        f32 = lambda k: float(np.float32(prm[k]))  # noqa: E731
        lib.temporal_moments_mirror_step(_f(rgb), index.ctypes.data_as(_I), _f(normal), _f(point), _f(pc), _f(pg), _f(pp), _f(pm),
                                         *(_f(a) for a in nxt), _f(out), _f(vout), _f(lout), _f(wout), w, h, int(self.has_history),
                                         int(static), _f(self.M), _f(self.fr), float(np.float32(spp)), f32("alpha_min"), f32("n_max"),
                                         f32("normal_cos_min"), float(r2), f32("w2_max"), f32("min_taps"))
        self.cur ^= 1
        self.has_history, self.key, self.last_static = True, key, static
        self.M, self.fr = mf
        return out.reshape(h, w, 3), vout.reshape(h, w, 3), lout.reshape(h, w), wout.reshape(h, w)
