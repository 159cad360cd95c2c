"""The CPU side of the tests of temporal accumulation's resampling mode: builds tests/temporal_cubic_mirror.cpp
— the plain step (§4.15) and the moments step (§4.16), each with a `mode` argument — with `g++ -O2 -ffp-contract=off`, as
tests/temporal_ref.py builds its mirror, and runs it on numpy arrays.  `Temporal` and `TemporalMoments` are the handle's state
machines around it, as tests/temporal_ref.py's and tests/temporal_moments_ref.py's are, with `resampling` ("bilinear" / "cubic"),
which may be changed between any two steps, and `taken`: the uint8 (height, width) array of the last step.  The host part of a step
(the camera's matrix) is §4.15's and comes from tests/temporal_ref.py."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import temporal_moments_ref
import temporal_ref
from temporal_ref import camera_key, camera_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULTS = dict(temporal_ref.DEFAULTS)
MOMENTS_DEFAULTS = dict(temporal_moments_ref.MOMENTS_DEFAULTS)
MODES = {"bilinear": 0, "cubic": 1}  # RAYZ_TEMPORAL_RESAMPLE_*

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
        raise RuntimeError("no g++: the resampling mode's CPU mirror cannot be built")
    so = os.path.join(tempfile.mkdtemp(prefix="temporal_cubic_mirror_"), "temporal_cubic_mirror.so")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "temporal_cubic_mirror.cpp")], check=True, capture_output=True, timeout=300)
    lib = C.CDLL(so)
    lib.temporal_cubic_mirror_step.argtypes = [_F, _F, _I, _F, _F] + [_F] * 8 + [_F, _F, _F, C.c_uint32, C.c_uint32, C.c_int, C.c_int, _F, _F] + \
        [C.c_float] * 5 + [C.c_int, _B]
    lib.temporal_cubic_mirror_step.restype = None
    lib.temporal_cubic_mirror_step_moments.argtypes = [_F, _I, _F, _F] + [_F] * 9 + \
        [_F, _F, _F, _F, C.c_uint32, C.c_uint32, C.c_int, C.c_int, _F, _F] + [C.c_float] * 7 + [C.c_int, _B]
    lib.temporal_cubic_mirror_step_moments.restype = None
    lib.temporal_cubic_mirror_weights.argtypes = [C.c_float, _F]
    lib.temporal_cubic_mirror_weights.restype = None
    _lib = lib
    return lib


def _f(a):
    return a.ctypes.data_as(_F)


def weights(f):
    """§4.26's four weights of f (w-1, w0, w1, w2) as float32."""
    w = np.empty(4, np.float32)
    load().temporal_cubic_mirror_weights(float(np.float32(f)), _f(w))
    return w


class _Handle:
    RECORDS = 4

    def __init__(self, width, height, resampling="bilinear"):
        self.width, self.height = width, height
        n = width * height
        self.hist = [[np.zeros((n, 4), np.float32) for _ in range(self.RECORDS)] for _ in range(2)]
        self.cur = 0
        self.has_history = False
        self.key = None
        self.M, self.fr = np.zeros(9, np.float32), np.zeros(3, np.float32)
        self.last_static = None
        self.resampling = resampling
        self.taken = None

    def reset(self):
        self.has_history = False

    def state(self):
        h, w = self.height, self.width
        return tuple(a.reshape(h, w, 4).copy() for a in self.hist[self.cur])

    def _begin(self, camera, prm):
        mf = camera_matrix(camera)
        if mf is None:
            raise ValueError("camera: det is 0 or not finite")
        key = camera_key(camera)
        static = self.has_history and key == self.key
        with np.errstate(over="ignore"):
            r = np.float32(prm["max_rel_dist"])
            r2 = r * r
        return mf, key, static, float(r2)

    def _end(self, mf, key, static, taken):
        self.cur ^= 1
        self.has_history, self.key, self.last_static = True, key, static
        self.M, self.fr = mf
        self.taken = taken.reshape(self.height, self.width)


class Temporal(_Handle):
    """The mirror's plain handle: `step` is rayz_hip_temporal_step on numpy arrays in the handle's `resampling`; returns (colour,
    variance, length).  `state()`: (c, v, g, p), each (h, w, 4) float32."""

    def step(self, rgb, var_rgb, index, normal, point, camera, spp, **params):
        lib = load()
        prm = {**DEFAULTS, **params}
        h, w = self.height, self.width
        n = h * w
        mf, key, static, r2 = self._begin(camera, prm)
        rgb, var_rgb, normal, point = (np.ascontiguousarray(a, dtype=np.float32).reshape(n, 3) for a in (rgb, var_rgb, normal, point))
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(n)
        prev, nxt = self.hist[self.cur], self.hist[self.cur ^ 1]
        out, vout, lout = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty(n, np.float32)
        taken = np.full(n, 255, np.uint8)
        f32 = lambda k: float(np.float32(prm[k]))  # noqa: E731
        lib.temporal_cubic_mirror_step(_f(rgb), _f(var_rgb), index.ctypes.data_as(_I), _f(normal), _f(point), *(_f(a) for a in prev),
                                       *(_f(a) for a in nxt), _f(out), _f(vout), _f(lout), w, h, int(self.has_history), int(static),
                                       _f(self.M), _f(self.fr), float(np.float32(spp)), f32("alpha_min"), f32("n_max"),
                                       f32("normal_cos_min"), r2, MODES[self.resampling], taken.ctypes.data_as(_B))
        self._end(mf, key, static, taken)
        return out.reshape(h, w, 3), vout.reshape(h, w, 3), lout.reshape(h, w)


class TemporalMoments(_Handle):
    """The mirror's handle in moments mode: `step` is rayz_hip_temporal_step_moments in the handle's `resampling`; returns (colour,
    variance, length, W2).  `state()`: (c, v, g, p, m)."""
    RECORDS = 5

    def step(self, rgb, index, normal, point, camera, spp, **params):
        lib = load()
        unknown = set(params) - set(DEFAULTS) - set(MOMENTS_DEFAULTS)
        assert not unknown, unknown
        prm = {**DEFAULTS, **MOMENTS_DEFAULTS, **params}
        h, w = self.height, self.width
        n = h * w
        mf, key, static, r2 = self._begin(camera, prm)
        rgb, normal, point = (np.ascontiguousarray(a, dtype=np.float32).reshape(n, 3) for a in (rgb, normal, point))
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(n)
        (pc, _, pg, pp, pm), nxt = self.hist[self.cur], self.hist[self.cur ^ 1]
        out, vout = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        lout, wout = np.empty(n, np.float32), np.empty(n, np.float32)
        taken = np.full(n, 255, np.uint8)
        f32 = lambda k: float(np.float32(prm[k]))  # noqa: E731
        lib.temporal_cubic_mirror_step_moments(_f(rgb), index.ctypes.data_as(_I), _f(normal), _f(point), _f(pc), _f(pg), _f(pp), _f(pm),
                                               *(_f(a) for a in nxt), _f(out), _f(vout), _f(lout), _f(wout), w, h, int(self.has_history),
                                               int(static), _f(self.M), _f(self.fr), float(np.float32(spp)), f32("alpha_min"),
                                               f32("n_max"), f32("normal_cos_min"), r2, f32("w2_max"), f32("min_taps"),
                                               MODES[self.resampling], taken.ctypes.data_as(_B))
        self._end(mf, key, static, taken)
        return out.reshape(h, w, 3), vout.reshape(h, w, 3), lout.reshape(h, w), wout.reshape(h, w)
