"""The CPU side of the tests of temporal accumulation's background mode: builds tests/temporal_background_mirror.cpp (the
restatement of DESIGN.md §4.27 on the plain, the moments and the two counts steps) with `g++ -O2 -ffp-contract=off`, as
tests/temporal_ref.py builds its mirror, and runs it on numpy arrays.  `Temporal` and `TemporalMoments` are the handles' state
machines around it — those of tests/temporal_ref.py and tests/temporal_moments_ref.py with a `background` mode ("input" or
"accumulate", settable between any two steps) and a `step` whose spp is an int (the scalar step) or an (h, w) array of per-pixel
counts (the counts step)."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import temporal_moments_ref
import temporal_ref
from temporal_ref import camera_fields, camera_key, camera_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULTS = dict(temporal_ref.DEFAULTS)
MOMENTS_DEFAULTS = dict(temporal_moments_ref.MOMENTS_DEFAULTS)
MODES = {"input": 0, "accumulate": 1}

_lib = None
_F = C.POINTER(C.c_float)
_D = C.POINTER(C.c_double)
_I = C.POINTER(C.c_int32)
_U = C.POINTER(C.c_uint32)


def load():
    global _lib
    if _lib is not None:
        return _lib
    gxx = shutil.which("g++")
    if not gxx:
        raise RuntimeError("no g++: the background mode's CPU mirror cannot be built")
    so = os.path.join(tempfile.mkdtemp(prefix="temporal_background_mirror_"), "temporal_background_mirror.so")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "temporal_background_mirror.cpp")], check=True, capture_output=True, timeout=300)
    lib = C.CDLL(so)
    lib.temporal_background_mirror_G.argtypes = [_D, _D, _F]
    lib.temporal_background_mirror_G.restype = None
    lib.temporal_background_mirror_step.argtypes = [_F, _F, _U, _I, _F, _F] + [_F] * 8 + [_F, _F, _F, C.c_uint32, C.c_uint32, C.c_int, C.c_int,
                                                                                          C.c_int, _F, _F, _F] + [C.c_float] * 5
    lib.temporal_background_mirror_step.restype = None
    lib.temporal_background_mirror_step_moments.argtypes = [_F, _U, _I, _F, _F] + [_F] * 9 + [_F, _F, _F, _F, C.c_uint32, C.c_uint32, C.c_int,
                                                                                             C.c_int, C.c_int, _F, _F, _F] + [C.c_float] * 7
    lib.temporal_background_mirror_step_moments.restype = None
    _lib = lib
    return lib


def _f(a):
    return a.ctypes.data_as(_F)


def background_matrix(prev_camera, camera):
    """§4.27's G (9,) float32: this frame's pixel centre (x, y, 1) to s·(x', y', 1) in the frame of `prev_camera`."""
    G = np.empty(9, np.float32)
    a, b = camera_fields(prev_camera), camera_fields(camera)
    with np.errstate(all="ignore"):
        load().temporal_background_mirror_G(a.ctypes.data_as(_D), b.ctypes.data_as(_D), _f(G))
    return G


def _counts(spp, h, w):
    """(None, f32 spp) for an int, (the (h·w,) uint32 array, 0.0) for an (h, w) array of non-negative integers."""
    if np.isscalar(spp):
        return None, float(np.float32(spp))
    spp = np.asarray(spp)
    assert spp.shape == (h, w) and (spp >= 0).all(), spp.shape
    return np.ascontiguousarray(spp.astype(np.uint32)).reshape(h * w), 0.0


class _Handle:
    RECORDS = 4

    def __init__(self, width, height, background="input"):
        self.width, self.height = width, height
        n = width * height
        self.hist = [[np.zeros((n, 4), np.float32) for _ in range(self.RECORDS)] for _ in range(2)]
        self.cur = 0
        self.has_history = False
        self.key = self.camera = None
        self.M, self.fr = np.zeros(9, np.float32), np.zeros(3, np.float32)
        self.last_static = None
        self.G = np.zeros(9, np.float32)  # the last step's, for the tests to look at
        self.set_background(background)

    def set_background(self, background):
        self.background = MODES[background]

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
        self.G = np.zeros(9, np.float32)
        if self.has_history and not static:
            self.G = background_matrix(self.camera, camera)
        return mf, key, static, float(r2)

    def _end(self, mf, key, static, camera):
        self.cur ^= 1
        self.has_history, self.key, self.last_static, self.camera = True, key, static, camera
        self.M, self.fr = mf


class Temporal(_Handle):
    """The mirror's plain handle: `step` is rayz_hip_temporal_step (spp an int) or _step_counts (spp an (h, w) array) and returns
    (colour, variance, length); `state()` is (c, v, g, p)."""

    def step(self, rgb, var_rgb, index, normal, point, camera, spp, **params):
        lib = load()
        assert not set(params) - set(DEFAULTS), params
        prm = {**DEFAULTS, **params}
        h, w = self.height, self.width
        n = h * w
        mf, key, static, r2 = self._begin(camera, prm)
        rgb, var_rgb, normal, point = (np.ascontiguousarray(a, dtype=np.float32).reshape(n, 3) for a in (rgb, var_rgb, normal, point))
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(n)
        cnt, s = _counts(spp, h, w)
        prev, nxt = self.hist[self.cur], self.hist[self.cur ^ 1]
        out, vout, lout = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty(n, np.float32)
        f32 = lambda k: float(np.float32(prm[k]))  # noqa: E731
        with np.errstate(all="ignore"):
            lib.temporal_background_mirror_step(_f(rgb), _f(var_rgb), cnt.ctypes.data_as(_U) if cnt is not None else None,
                                                index.ctypes.data_as(_I), _f(normal), _f(point), *(_f(a) for a in prev),
                                                *(_f(a) for a in nxt), _f(out), _f(vout), _f(lout), w, h, int(self.has_history), int(static),
                                                self.background, _f(self.M), _f(self.fr), _f(self.G), s, f32("alpha_min"), f32("n_max"),
                                                f32("normal_cos_min"), r2)
        self._end(mf, key, static, camera)
        return out.reshape(h, w, 3), vout.reshape(h, w, 3), lout.reshape(h, w)


class TemporalMoments(_Handle):
    """The mirror's moments handle: `step` is rayz_hip_temporal_step_moments or _step_moments_counts and returns (colour, variance,
    length, W2); `state()` is (c, v, g, p, m)."""

    RECORDS = 5

    def step(self, rgb, index, normal, point, camera, spp, **params):
        lib = load()
        assert not set(params) - set(DEFAULTS) - set(MOMENTS_DEFAULTS), params
        prm = {**DEFAULTS, **MOMENTS_DEFAULTS, **params}
        h, w = self.height, self.width
        n = h * w
        mf, key, static, r2 = self._begin(camera, prm)
        rgb, normal, point = (np.ascontiguousarray(a, dtype=np.float32).reshape(n, 3) for a in (rgb, normal, point))
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(n)
        cnt, s = _counts(spp, h, w)
        (pc, _, pg, pp, pm), nxt = self.hist[self.cur], self.hist[self.cur ^ 1]
        out, vout = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        lout, wout = np.empty(n, np.float32), np.empty(n, np.float32)
        f32 = lambda k: float(np.float32(prm[k]))  # noqa: E731
        with np.errstate(all="ignore"):
            lib.temporal_background_mirror_step_moments(_f(rgb), cnt.ctypes.data_as(_U) if cnt is not None else None,
                                                        index.ctypes.data_as(_I), _f(normal), _f(point), _f(pc), _f(pg), _f(pp), _f(pm),
                                                        *(_f(a) for a in nxt), _f(out), _f(vout), _f(lout), _f(wout), w, h,
                                                        int(self.has_history), int(static), self.background, _f(self.M), _f(self.fr),
                                                        _f(self.G), s, f32("alpha_min"), f32("n_max"), f32("normal_cos_min"), r2,
                                                        f32("w2_max"), f32("min_taps"))
        self._end(mf, key, static, camera)
        return out.reshape(h, w, 3), vout.reshape(h, w, 3), lout.reshape(h, w), wout.reshape(h, w)
