"""The CPU side of the tests of temporal accumulation's clip mode: builds tests/temporal_clip_mirror.cpp (the restatement of
DESIGN.md §4.28 on the plain and the moments step, in both background modes) with `g++ -O2 -ffp-contract=off`, as
tests/temporal_background_ref.py builds its mirror, and runs it on numpy arrays.  `Temporal` and `TemporalMoments` are that
module's state machines with a clip mode ("off" or "variance", its `gamma` and `min_taps`, settable between any two steps), a
`step` whose spp is an int, and `clipped`: the last step's uint8 (h, w) map."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import temporal_background_ref as bgref

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULTS = dict(bgref.DEFAULTS)
MOMENTS_DEFAULTS = dict(bgref.MOMENTS_DEFAULTS)
CLIP_DEFAULTS = {"gamma": 1.0, "min_taps": 4.0}
CLIP_MODES = {"off": 0, "variance": 1}

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
        raise RuntimeError("no g++: the clip mode's CPU mirror cannot be built")
    so = os.path.join(tempfile.mkdtemp(prefix="temporal_clip_mirror_"), "temporal_clip_mirror.so")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "temporal_clip_mirror.cpp")], check=True, capture_output=True, timeout=300)
    lib = C.CDLL(so)
    tail = [C.c_uint32, C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_int, _F, _F, _F]
    lib.temporal_clip_mirror_step.argtypes = [_F, _F, _I, _F, _F] + [_F] * 8 + [_F, _F, _F, _B] + tail + [C.c_float] * 7
    lib.temporal_clip_mirror_step.restype = None
    lib.temporal_clip_mirror_step_moments.argtypes = [_F, _I, _F, _F] + [_F] * 9 + [_F, _F, _F, _F, _B] + tail + [C.c_float] * 9
    lib.temporal_clip_mirror_step_moments.restype = None
    _lib = lib
    return lib


def _f(a):
    return a.ctypes.data_as(_F)


class _Clip:
    """What both handles add to tests/temporal_background_ref.py's: the clip mode and the last step's map."""

    def _init_clip(self, clip, gamma, min_taps):
        self.clipped = np.zeros((self.height, self.width), np.uint8)
        self.set_clip(clip, gamma, min_taps)

    def set_clip(self, clip, gamma=None, min_taps=None):
        self.clip = CLIP_MODES[clip]
        self.gamma = float(np.float32(CLIP_DEFAULTS["gamma"] if gamma is None else gamma))
        self.clip_min_taps = float(np.float32(CLIP_DEFAULTS["min_taps"] if min_taps is None else min_taps))


class Temporal(bgref._Handle, _Clip):
    """The mirror's plain handle: `step` is rayz_hip_temporal_step and returns (colour, variance, length); `state()` is (c, v, g, p)."""

    def __init__(self, width, height, background="input", clip="off", gamma=None, min_taps=None):
        bgref._Handle.__init__(self, width, height, background)
        self._init_clip(clip, gamma, min_taps)

    def step(self, rgb, var_rgb, index, normal, point, camera, spp, **params):
        lib = load()
        assert not set(params) - set(DEFAULTS), params
        prm = {**DEFAULTS, **params}
        h, w = self.height, self.width
        n = h * w
        mf, key, static, r2 = self._begin(camera, prm)
        rgb, var_rgb, normal, point = (np.ascontiguousarray(a, dtype=np.float32).reshape(n, 3) for a in (rgb, var_rgb, normal, point))
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(n)
        prev, nxt = self.hist[self.cur], self.hist[self.cur ^ 1]
        out, vout, lout = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty(n, np.float32)
        clipped = np.empty(n, np.uint8)
        f32 = lambda k: float(np.float32(prm[k]))  # noqa: E731
        with np.errstate(all="ignore"):
            lib.temporal_clip_mirror_step(_f(rgb), _f(var_rgb), index.ctypes.data_as(_I), _f(normal), _f(point), *(_f(a) for a in prev),
                                          *(_f(a) for a in nxt), _f(out), _f(vout), _f(lout), clipped.ctypes.data_as(_B), w, h,
                                          int(self.has_history), int(static), self.background, self.clip, _f(self.M), _f(self.fr),
                                          _f(self.G), float(np.float32(spp)), f32("alpha_min"), f32("n_max"), f32("normal_cos_min"), r2,
                                          self.gamma, self.clip_min_taps)
        self._end(mf, key, static, camera)
        self.clipped = clipped.reshape(h, w)
        return out.reshape(h, w, 3), vout.reshape(h, w, 3), lout.reshape(h, w)


class TemporalMoments(bgref._Handle, _Clip):
    """The mirror's moments handle: `step` is rayz_hip_temporal_step_moments and returns (colour, variance, length, W2); `state()`
    is (c, v, g, p, m)."""

    RECORDS = 5

    def __init__(self, width, height, background="input", clip="off", gamma=None, min_taps=None):
        bgref._Handle.__init__(self, width, height, background)
        self._init_clip(clip, gamma, min_taps)

    def step(self, rgb, index, normal, point, camera, spp, **params):
        lib = load()
        assert not set(params) - set(DEFAULTS) - set(MOMENTS_DEFAULTS), params
        prm = {**DEFAULTS, **MOMENTS_DEFAULTS, **params}
        h, w = self.height, self.width
        n = h * w
        mf, key, static, r2 = self._begin(camera, prm)
        rgb, normal, point = (np.ascontiguousarray(a, dtype=np.float32).reshape(n, 3) for a in (rgb, normal, point))
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(n)
        (pc, _, pg, pp, pm), nxt = self.hist[self.cur], self.hist[self.cur ^ 1]
        out, vout = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        lout, wout = np.empty(n, np.float32), np.empty(n, np.float32)
        clipped = np.empty(n, np.uint8)
        f32 = lambda k: float(np.float32(prm[k]))  # noqa: E731
        with np.errstate(all="ignore"):
            lib.temporal_clip_mirror_step_moments(_f(rgb), index.ctypes.data_as(_I), _f(normal), _f(point), _f(pc), _f(pg), _f(pp), _f(pm),
                                                  *(_f(a) for a in nxt), _f(out), _f(vout), _f(lout), _f(wout),
                                                  clipped.ctypes.data_as(_B), w, h, int(self.has_history), int(static), self.background,
                                                  self.clip, _f(self.M), _f(self.fr), _f(self.G), float(np.float32(spp)), f32("alpha_min"),
                                                  f32("n_max"), f32("normal_cos_min"), r2, f32("w2_max"), f32("min_taps"), self.gamma,
                                                  self.clip_min_taps)
        self._end(mf, key, static, camera)
        self.clipped = clipped.reshape(h, w)
        return out.reshape(h, w, 3), vout.reshape(h, w, 3), lout.reshape(h, w), wout.reshape(h, w)
