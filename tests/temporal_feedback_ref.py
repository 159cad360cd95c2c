"""The CPU side of the tests of temporal accumulation's feedback mode: builds tests/temporal_feedback_mirror.cpp (the restatement
of DESIGN.md §4.17) with `g++ -O2 -ffp-contract=off`, as tests/temporal_moments_ref.py builds its mirror, and runs it on numpy
arrays.  `TemporalFeedback` is the handle's state machine around it: two history buffers of five records (c, m1, g, p, m), the
previous camera (its matrix from tests/temporal_ref.py: the host part of a step is §4.15's), the "has history" flag, and which side
the last step wrote — the side `feedback` writes to.  `variant`: a named misreading of §4.17 (see the mirror), 0 for the section."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

import temporal_moments_ref
from temporal_ref import camera_key, camera_matrix

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULTS = dict(temporal_moments_ref.DEFAULTS)
MOMENTS_DEFAULTS = dict(temporal_moments_ref.MOMENTS_DEFAULTS)
VARIANTS = {1: "variance from the fed-back colour", 2: "feedback also overwrites m1", 3: "feedback overwrites N",
            4: "feedback written to the older side", 5: "m1 from the pixel's own record instead of the taps",
            6: "non-finite feedback stored"}

_lib = None
_F = C.POINTER(C.c_float)
_I = C.POINTER(C.c_int32)


def load():
    global _lib
    if _lib is not None:
        return _lib
    gxx = shutil.which("g++")
    if not gxx:
        raise RuntimeError("no g++: the feedback mode's CPU mirror cannot be built")
    so = os.path.join(tempfile.mkdtemp(prefix="temporal_feedback_mirror_"), "temporal_feedback_mirror.so")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "temporal_feedback_mirror.cpp")], check=True, capture_output=True, timeout=300)
    lib = C.CDLL(so)
    lib.temporal_feedback_mirror_step.argtypes = [_F, _I, _F, _F] + [_F] * 10 + [_F, _F, _F, _F, C.c_uint32, C.c_uint32, C.c_int, C.c_int, _F, _F] + \
        [C.c_float] * 7 + [C.c_int]
    lib.temporal_feedback_mirror_step.restype = None
    lib.temporal_feedback_mirror_write.argtypes = [_F, _F, _F, C.c_uint32, C.c_uint32, C.c_int]
    lib.temporal_feedback_mirror_write.restype = None
    _lib = lib
    return lib


def _f(a):
    return a.ctypes.data_as(_F)


class TemporalFeedback:
    """The mirror's feedback handle: `step` is rayz_hip_temporal_step_moments on a handle that tracks feedback, on numpy arrays, and
    returns (colour, variance, length, W2); `feedback` is rayz_hip_temporal_feedback (ValueError where the library says
    RAYZ_ERR_STATE); `reset` is rayz_hip_temporal_reset.  `state()` returns the history the last step left, with what feedback did
    to it: (c, m1, g, p, m), each (h, w, 4) float32, the index as bits in g[..., 3], m = {m2, W2}."""

    def __init__(self, width, height, variant=0):
        self.width, self.height, self.variant = width, height, variant
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

    def feedback(self, rgb):
        if not self.has_history:
            raise ValueError("no history to write to")
        side = self.hist[self.cur ^ 1] if self.variant == 4 else self.hist[self.cur]
        img = np.ascontiguousarray(rgb, dtype=np.float32).reshape(self.width * self.height, 3)
        load().temporal_feedback_mirror_write(_f(side[0]), _f(side[1]), _f(img), self.width, self.height, self.variant)

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
        prev, nxt = self.hist[self.cur], self.hist[self.cur ^ 1]
        out, vout = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32)
        lout, wout = np.empty(n, np.float32), np.empty(n, np.float32)
        with np.errstate(over="ignore"):
            r = np.float32(prm["max_rel_dist"])
            r2 = r * r
        f32 = lambda k: float(np.float32(prm[k]))  # noqa: E731
        lib.temporal_feedback_mirror_step(_f(rgb), index.ctypes.data_as(_I), _f(normal), _f(point), *(_f(a) for a in prev),
                                          *(_f(a) for a in nxt), _f(out), _f(vout), _f(lout), _f(wout), w, h, int(self.has_history),
                                          int(static), _f(self.M), _f(self.fr), float(np.float32(spp)), f32("alpha_min"), f32("n_max"),
                                          f32("normal_cos_min"), float(r2), f32("w2_max"), f32("min_taps"), self.variant)
        self.cur ^= 1
        self.has_history, self.key, self.last_static = True, key, static
        self.M, self.fr = mf
        return out.reshape(h, w, 3), vout.reshape(h, w, 3), lout.reshape(h, w), wout.reshape(h, w)
