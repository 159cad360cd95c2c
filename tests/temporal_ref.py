"""The CPU side of temporal accumulation's tests: builds tests/temporal_mirror.cpp (the restatement of DESIGN.md §4.15, the host
part included) with `g++ -O2 -ffp-contract=off`, as tests/denoise_guided_ref.py builds the guided mirror, and runs it on numpy
arrays.  `Temporal` is the handle's state machine around it: two history buffers, the previous camera, the "has history" flag."""
import ctypes as C
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DEFAULTS = {"alpha_min": 0.05, "n_max": 65536.0, "normal_cos_min": 0.9, "max_rel_dist": 0.05}  # RAYZ_TEMPORAL_DEFAULT_*
VCAP = np.float32(2.0 ** 32)

_lib = None
_F = C.POINTER(C.c_float)
_D = C.POINTER(C.c_double)
_I = C.POINTER(C.c_int32)


def load():
    global _lib
    if _lib is not None:
        return _lib
    gxx = shutil.which("g++")
    if not gxx:
        raise RuntimeError("no g++: the temporal accumulation's CPU mirror cannot be built")
    so = os.path.join(tempfile.mkdtemp(prefix="temporal_mirror_"), "temporal_mirror.so")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "temporal_mirror.cpp")], check=True, capture_output=True, timeout=300)
    lib = C.CDLL(so)
    lib.temporal_mirror_camera.argtypes = [_D, _F, _F]
    lib.temporal_mirror_camera.restype = C.c_int
    lib.temporal_mirror_step.argtypes = [_F, _F, _I, _F, _F] + [_F] * 8 + [_F, _F, _F, C.c_uint32, C.c_uint32, C.c_int, C.c_int, _F, _F] + \
        [C.c_float] * 5
    lib.temporal_mirror_step.restype = None
    lib.temporal_mirror_project.argtypes = [_F, C.c_size_t, _F, _F, _F]
    lib.temporal_mirror_project.restype = None
    _lib = lib
    return lib


def _f(a):
    return a.ctypes.data_as(_F)


def camera_fields(cam):
    """The twelve doubles of a camera that §4.15 reads — look_from, px_du, px_dv, px_origin — from a capi.CameraDesc or from a dict
    / object with those names."""
    get = (lambda k: cam[k]) if isinstance(cam, dict) else (lambda k: getattr(cam, k))
    return np.array([list(get(k)) for k in ("look_from", "px_du", "px_dv", "px_origin")], np.float64).reshape(12)


def camera_key(cam):
    """All 152 bytes of the RayzCameraDesc a camera stands for: what "the same camera" compares."""
    get = (lambda k, d: cam.get(k, d)) if isinstance(cam, dict) else (lambda k, d: getattr(cam, k, d))
    vecs = [np.array(list(get(k, (0.0, 0.0, 0.0))), np.float64) for k in ("look_from", "px_du", "px_dv", "px_origin", "defocus_u", "defocus_v")]
    return b"".join(v.tobytes() for v in vecs) + np.array([int(get("defocus", 0)), int(get("_pad", 0))], np.uint32).tobytes()


def camera_matrix(cam):
    """(M (9,) f32, from (3,) f32), or None where det is zero or not finite (RAYZ_ERR_BAD_ARG)."""
    c = camera_fields(cam)
    M, fr = np.empty(9, np.float32), np.empty(3, np.float32)
    ok = load().temporal_mirror_camera(c.ctypes.data_as(_D), _f(M), _f(fr))
    return (M, fr) if ok else None


def project(points, M, fr):
    """The f32 (x, y, γ) of §4.15's step 2 for points (n, 3) float32 through `M`, `fr` of camera_matrix: (n, 3) float32."""
    points = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    out = np.empty_like(points)
    with np.errstate(all="ignore"):
        load().temporal_mirror_project(_f(points), len(points), _f(M), _f(fr), _f(out))
    return out


class Temporal:
    """The mirror's handle: `step` is rayz_hip_temporal_step on numpy arrays, `reset` rayz_hip_temporal_reset.  `state()` returns the
    history the last step left: (c (h, w, 4), v (h, w, 4), g (h, w, 4), p (h, w, 4)) float32, the index as bits in g[..., 3]."""

    def __init__(self, width, height):
        self.width, self.height = width, height
        n = width * height
        self.hist = [[np.zeros((n, 4), np.float32) for _ in range(4)] for _ in range(2)]
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

    def step(self, rgb, var_rgb, index, normal, point, camera, spp, length=True, **params):
        lib = load()
        prm = {**DEFAULTS, **params}
        h, w = self.height, self.width
        n = h * w
        mf = camera_matrix(camera)
        if mf is None:
            raise ValueError("camera: det is 0 or not finite")
        rgb, var_rgb, normal, point = (np.ascontiguousarray(a, dtype=np.float32).reshape(n, 3) for a in (rgb, var_rgb, normal, point))
        index = np.ascontiguousarray(index, dtype=np.int32).reshape(n)
        key = camera_key(camera)
        static = self.has_history and key == self.key
        prev, nxt = self.hist[self.cur], self.hist[self.cur ^ 1]
        out, vout, lout = np.empty((n, 3), np.float32), np.empty((n, 3), np.float32), np.empty(n, np.float32)
        with np.errstate(over="ignore"):
            r = np.float32(prm["max_rel_dist"])
            r2 = r * r
        lib.temporal_mirror_step(_f(rgb), _f(var_rgb), index.ctypes.data_as(_I), _f(normal), _f(point), *(_f(a) for a in prev),
                                 *(_f(a) for a in nxt), _f(out), _f(vout), _f(lout) if length else None, w, h, int(self.has_history),
                                 int(static), _f(self.M), _f(self.fr), float(np.float32(spp)), float(np.float32(prm["alpha_min"])),
                                 float(np.float32(prm["n_max"])), float(np.float32(prm["normal_cos_min"])), float(r2))
        self.cur ^= 1
        self.has_history, self.key, self.last_static = True, key, static
        self.M, self.fr = mf
        res = (out.reshape(h, w, 3), vout.reshape(h, w, 3))
        return res + (lout.reshape(h, w),) if length else res
