"""Device-resident rendering through the C ABI (include/rayz_hip.h).

`DeviceScene` keeps the flattened pool in HBM and renders shards into GPU buffers the caller owns
(torch tensors in bench.py and the tests) — the split form of `Tracer.render()` that keeps uploads,
allocation and the host copy out of the timed region.
"""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np

from . import capi


_default_device = None  # the ordinal of the last successful init(): where a scene created without a device is bound


def init(device: int = 0) -> None:
    global _default_device
    lib = capi.load()
    capi.check(lib, lib.rayz_hip_init(device), f"rayz_hip_init({device})")
    _default_device = device


def debug_set(knob: int, value: int = -1) -> None:
    """`rayz_hip_debug_set`: a measurement knob (scheduling / walked tree; never an image); value < 0 = default."""
    lib = capi.load()
    capi.check(lib, lib.rayz_hip_debug_set(knob, value), f"rayz_hip_debug_set({knob})")


def shard_rows(params: capi.RenderParams) -> int:
    return int(capi.load().rayz_hip_shard_rows(C.byref(params)))


def shard_row_indices(height: int, tile_rows: int, shard_index: int, shard_count: int) -> np.ndarray:
    """Global row numbers of a shard's compact output, in order (host-side bookkeeping of the gather)."""
    tile_rows = tile_rows or 8  # RAYZ_DEFAULT_TILE_ROWS
    shard_count = shard_count or 1
    rows = np.arange(height)
    return rows[(rows // tile_rows) % shard_count == shard_index]


def render_host(scene: capi.SceneDesc, camera: capi.CameraDesc, params: capi.RenderParams):
    """One-shot blocking render into host memory: `rayz_hip_render[_f64]`.  Returns (image, stats)."""
    lib = capi.load()
    rows = shard_rows(params)
    f64 = params.precision == capi.PRECISION_F64
    out = np.empty((rows, params.width, 3), dtype=np.float64 if f64 else np.float32)
    st = capi.RenderStats()
    fn = lib.rayz_hip_render_f64 if f64 else lib.rayz_hip_render
    rc = fn(C.byref(scene), C.byref(camera), C.byref(params), out.ctypes.data_as(C.c_void_p), C.byref(st))
    capi.check(lib, rc, "rayz_hip_render")
    return out, st


class _Handle:
    """Owns a library handle: `_h`, `close()` and `__del__`.  A class names the library function that destroys its handle (and waits
    for the handle's last work) in `_destroy`."""

    _destroy = None
    _h = None

    def close(self) -> None:
        if self._h:
            getattr(self._lib, self._destroy)(self._h)
            self._h = C.c_void_p()
        self._inflight = None  # (tensors a handle kept alive for its last call)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _check_tensor(name, t, dtype, shape, device, owner) -> None:
    """`t` is a contiguous torch tensor of `dtype` and `shape` in the memory of GPU `device`, where `owner` ("the denoiser") lives."""
    import torch

    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"{name} must be a torch tensor in GPU memory")
    if t.device.index != device:
        raise ValueError(f"{name} is on cuda:{t.device.index}, {owner} on cuda:{device}")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if tuple(t.shape) != shape:
        raise ValueError(f"{name} must be {shape}, got {tuple(t.shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")


def _params(struct, defaults, given, what):
    """`struct(**defaults)` with the fields `given` names replaced; `what` ("denoise") names the parameters in the refusal."""
    unknown = set(given) - set(defaults)
    if unknown:
        raise ValueError(f"unknown {what} parameter(s) {sorted(unknown)}; choose from {sorted(defaults)}")
    return struct(**{**defaults, **given})


def _check_frame_tensors(owner, device, frame, inputs, gbuffer, need, outputs) -> None:
    """A frame filter's tensors in argument order: the float32 `inputs` [(name, tensor)] shaped `frame`, the guides `need` names (index
    is int32 (height, width), the others float32 frames) and the float32 `outputs` [(name, tensor, shape)], a None among them not
    being asked for."""
    import torch

    tensors = [(name, t, torch.float32, frame) for name, t in inputs]
    tensors += [(f"gbuffer.{k}", getattr(gbuffer, k), torch.int32 if k == "index" else torch.float32, frame[:2] if k == "index" else frame)
                for k in need]
    tensors += [(name, t, torch.float32, shape) for name, t, shape in outputs if t is not None]
    for t in tensors:
        _check_tensor(*t, device, owner)


def _gbuffer_pointers(gbuffer, need) -> capi.QueryOutputs:
    o = capi.QueryOutputs()
    for k in need:
        setattr(o, k, getattr(gbuffer, k).data_ptr())
    return o


def _stream_prologue(stream: int, device: int) -> None:
    import torch

    if not stream:  # the library's stream does not order itself after torch's
        torch.cuda.synchronize(device)


def _optional_out(out, shape, device):
    """The optional-output convention: True for a new float32 tensor of `shape`, False for none, or the caller's tensor."""
    import torch

    if out is True:
        return torch.empty(shape, dtype=torch.float32, device=device)
    return None if out is False else out


QUERY_OUTPUTS = ("index", "t", "point", "normal", "front_face", "material", "albedo")
CHAIN_OUTPUTS = ("key", "depth", "first_index")  # what a chain G-buffer carries beside them (DeviceScene.gbuffer(chain=...))


class QueryResult:
    """The outputs of a query as torch tensors on the scene's device (None where not requested): index, material (int32),
    t (R), point / normal / albedo (..., 3) of R, front_face and hit (uint8).  Written asynchronously: call
    DeviceScene.query_sync() (or synchronise the stream) before reading them on the host.
    A chain G-buffer (`is_chain`, DeviceScene.gbuffer(chain=...)) holds the record of the LAST segment of every
    pixel's specular chain, and also key (int32: the chain key's 32 bits), depth (uint8) and first_index (int32)."""

    _VEC = ("point", "normal", "albedo")

    def __init__(self):
        for k in QUERY_OUTPUTS + ("hit",) + CHAIN_OUTPUTS:
            setattr(self, k, None)
        self.is_chain = False

    @classmethod
    def _alloc(cls, shape, dtype, device, outputs):
        import torch

        r = cls()
        for k in outputs:
            if k not in QUERY_OUTPUTS + ("hit",):
                raise ValueError(f"unknown query output {k!r}; choose from {QUERY_OUTPUTS + ('hit',)}")
            if k in ("index", "material"):
                t = torch.empty(shape, dtype=torch.int32, device=device)
            elif k in ("front_face", "hit"):
                t = torch.empty(shape, dtype=torch.uint8, device=device)
            elif k in cls._VEC:
                t = torch.empty(tuple(shape) + (3,), dtype=dtype, device=device)
            else:
                t = torch.empty(shape, dtype=dtype, device=device)
            setattr(r, k, t)
        return r

    def lattice(self, f: int, phase) -> "QueryResult":
        """The G-buffer of the lattice frame `lattice_pixels(width, height, f, phase)` renders: every field present, strided
        `[py::f, px::f]` and made contiguous.  A lattice sample is a pixel of this frame, so its guides are this frame's own."""
        px, py = _check_phase(f, phase)
        r = QueryResult()
        for k in QUERY_OUTPUTS + ("hit",) + CHAIN_OUTPUTS:
            t = getattr(self, k)
            if t is not None:
                setattr(r, k, t[py::f, px::f].contiguous())
        r.is_chain = self.is_chain
        return r

    def with_albedo(self, albedo) -> "QueryResult":
        """A copy of this G-buffer whose `albedo` is the given tensor — e.g. a sampled G-buffer's (DeviceScene.gbuffer_sampled,
        DESIGN.md §4.25), so that a filter's DENOISE_ALBEDO divides and multiplies by the mean over the frame's own camera rays.
        `albedo` must have the shape, dtype and device of this result's albedo (which must be present); every other field is
        shared with this result, not copied."""
        import torch

        if self.albedo is None:
            raise ValueError("with_albedo: this result carries no albedo to take the place of")
        if not isinstance(albedo, torch.Tensor) or albedo.device != self.albedo.device:
            raise ValueError(f"with_albedo: albedo must be a torch tensor on {self.albedo.device}")
        if albedo.dtype != self.albedo.dtype or tuple(albedo.shape) != tuple(self.albedo.shape) or not albedo.is_contiguous():
            raise ValueError(f"with_albedo: albedo must be contiguous {self.albedo.dtype} {tuple(self.albedo.shape)}, "
                             f"got {albedo.dtype} {tuple(albedo.shape)}")
        r = QueryResult()
        for k in QUERY_OUTPUTS + ("hit",) + CHAIN_OUTPUTS:
            setattr(r, k, getattr(self, k))
        r.is_chain = self.is_chain
        r.albedo = albedo
        return r

    def _outputs(self) -> capi.QueryOutputs:
        o = capi.QueryOutputs()
        for k in QUERY_OUTPUTS + ("hit",):
            t = getattr(self, k)
            if t is not None and t.numel():
                setattr(o, k, t.data_ptr())
        return o


SAMPLED_OUTPUTS = ("albedo", "normal", "t", "hits")


class SampledResult:
    """The outputs of DeviceScene.gbuffer_sampled as torch tensors on the scene's device, None where not
    requested: albedo and normal (rows, width, 3) and t (rows, width) of R — means over the pixel's samples, the normal not
    normalised —, hits (rows, width) int32 (the count's 32 bits), and `samples`, the n they are means over.  Written
    asynchronously: call DeviceScene.query_sync() before reading them on the host."""

    def __init__(self):
        for k in SAMPLED_OUTPUTS:
            setattr(self, k, None)
        self.samples = 0


class DeviceScene(_Handle):
    """A pool resident in HBM (`rayz_hip_scene_create`; `device` binds it to that HIP ordinal now)."""

    _destroy = "rayz_hip_scene_destroy"  # (waits for the scene's last launch)

    def __init__(self, scene: capi.SceneDesc, device: int | None = None):
        self._lib = capi.load()
        self._h = C.c_void_p()
        if device is None:
            rc = self._lib.rayz_hip_scene_create(C.byref(scene), C.byref(self._h))
        else:
            rc = self._lib.rayz_hip_scene_create_on(device, C.byref(scene), C.byref(self._h))
        capi.check(self._lib, rc, "rayz_hip_scene_create")
        self._device = device
        self._inflight = None  # (rays, outputs) of the last query: kept alive until query_sync (the kernel may still use them)
        self._sparse_inflight = None  # the tensors of the last render_pixels: kept alive until sync()

    @property
    def device(self) -> int:
        """The HIP ordinal the scene lives on (a scene created without one: the default device of init())."""
        d = self._device if self._device is not None else _default_device
        if d is None:
            raise capi.RayzHipError("no device: call render.init() first")
        return d

    def _query_prologue(self, stream: int):
        """Before a query: the previous one is waited for (its tensors released), and — on the library's own stream, which does not
        order itself after torch's — torch's work on the scene's device is finished, so the rays and outputs are in place."""
        import torch

        if self._inflight is not None:
            self.query_sync()
        if not stream:
            torch.cuda.synchronize(self.device)

    def render_into(self, camera: capi.CameraDesc, params: capi.RenderParams, out_ptr: int, stream: int = 0) -> None:
        """Asynchronous on `stream` (a hipStream_t as int, 0 = the library's stream); `out_ptr` is device memory."""
        fn = (self._lib.rayz_hip_render_device_f64 if params.precision == capi.PRECISION_F64
              else self._lib.rayz_hip_render_device)
        rc = fn(self._h, C.byref(camera), C.byref(params), C.c_void_p(out_ptr), C.c_void_p(stream))
        capi.check(self._lib, rc, "rayz_hip_render_device")

    def progressive(self, camera: capi.CameraDesc, params: capi.RenderParams, track_noise: bool = False, adaptive: bool = False,
                    min_chunks: int | None = None) -> "Progressive":
        """The frame of `render_into(camera, params, ...)` in passes of whole chunks (`rayz_hip_progressive_create`);
        `track_noise` makes it a tracked handle (`Progressive.noise`, `Progressive.render_until`), `adaptive` an adaptive one
        (`Progressive.adaptive_step`, `Progressive.render_adaptive`: DESIGN.md §4.14) that freezes no pixel before `min_chunks`
        chunks (default capi.ADAPTIVE_DEFAULT_MIN_CHUNKS)."""
        return Progressive(self, camera, params, track_noise=track_noise, adaptive=adaptive, min_chunks=min_chunks)

    def render_pixels(self, camera: capi.CameraDesc, params: capi.RenderParams, pixels, dest=None, out=None, var=False, stream: int = 0):
        """A sparse render (`rayz_hip_scene_render_pixels`): traces the listed pixels only, each to the bits
        `render_into(camera, params, ...)` gives it.  `pixels`: an int32 torch tensor (n,) on the scene's device, LOCAL row-major
        pixels of `params`' shard (row * width + column) in any order, duplicates allowed.  Without `dest` entry j goes to row j of
        `out`, shaped (n, 3) (allocated when None).  With `dest` (int32, (n,)) entry j goes to pixel slot dest[j] of `out`, which
        must be given: any contiguous tensor of (..., 3) in `params`' precision, e.g. a frame; slots nobody names keep their bits.
        `var`: True or a float32 tensor shaped as `out` for the per-channel variance of the mean at the same slots (True: a new
        tensor, NaN where nothing was written).  Returns `out`, or (out, var).  Blocks for the list's range check — an entry out of
        range is refused with nothing written — then runs asynchronously on `stream`; the tensors are kept alive by the scene until
        sync(), which returns this call's counters."""
        import torch

        dev = torch.device("cuda", self.device)
        dtype = torch.float64 if params.precision == capi.PRECISION_F64 else torch.float32
        for name, t in (("pixels", pixels), ("dest", dest)):
            if t is not None:
                _check_tensor(name, t, torch.int32, (int(pixels.numel()) if isinstance(pixels, torch.Tensor) else 0,), self.device, "the scene")
        n = int(pixels.numel())
        if out is None:
            if dest is not None:
                raise ValueError("dest scatters into a frame of the caller's: pass it as `out`")
            out = torch.empty((n, 3), dtype=dtype, device=dev)
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.device.index != self.device:
            raise ValueError(f"out must be a torch tensor on cuda:{self.device}")
        if out.dtype != dtype or not out.is_contiguous() or out.dim() < 2 or out.shape[-1] != 3:
            raise ValueError(f"out must be a contiguous {dtype} tensor shaped (..., 3), got {out.dtype} {tuple(out.shape)}")
        if var is True:
            var = torch.full(tuple(out.shape), float("nan"), dtype=torch.float32, device=dev)
        elif var is False:
            var = None
        if var is not None:
            _check_tensor("var", var, torch.float32, tuple(out.shape), self.device, "the scene")
        _stream_prologue(stream, self.device)
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)  # noqa: E731
        fn = self._lib.rayz_hip_scene_render_pixels_f64 if dtype == torch.float64 else self._lib.rayz_hip_scene_render_pixels
        rc = fn(self._h, C.byref(camera), C.byref(params), ptr(pixels), n, ptr(dest), out.numel() // 3, ptr(out), ptr(var),
                C.c_void_p(stream or None))
        capi.check(self._lib, rc, "rayz_hip_scene_render_pixels")
        self._sparse_inflight = (pixels, dest, out, var)
        return out if var is None else (out, var)

    def sync(self) -> capi.RenderStats:
        st = capi.RenderStats()
        capi.check(self._lib, self._lib.rayz_hip_scene_sync(self._h, C.byref(st)), "rayz_hip_scene_sync")
        self._sparse_inflight = None
        return st

    @property
    def scan_form(self) -> int:
        """The basis the next flat-list render's reject test runs in: capi.SCAN_FORM_XZ, _XY or _ONE_RADIUS (what AUTO chose, if
        nothing was set: _ONE_RADIUS is XY with the scene's one-radius sets in their own loop, where they are large enough)."""
        form = C.c_uint32()
        capi.check(self._lib, self._lib.rayz_hip_scene_get_scan_form(self._h, C.byref(form)), "rayz_hip_scene_get_scan_form")
        return form.value

    @scan_form.setter
    def scan_form(self, form: int) -> None:
        capi.check(self._lib, self._lib.rayz_hip_scene_set_scan_form(self._h, form), "rayz_hip_scene_set_scan_form")

    def set_primary_lists(self, mode: int) -> None:
        """capi.PRIMARY_LISTS_AUTO, _OFF or _ON: whether flat-list renders resolve each path's camera segment from its pixel's
        primary list instead of a scan; the frame is the same either way."""
        capi.check(self._lib, self._lib.rayz_hip_scene_set_primary_lists(self._h, mode), "rayz_hip_scene_set_primary_lists")

    def uses_primary_lists(self, samples_per_px: int) -> bool:
        """Whether a flat-list launch of that many samples per pixel would use the lists (what AUTO decides, if nothing was set)."""
        on = C.c_uint32()
        capi.check(self._lib, self._lib.rayz_hip_scene_get_primary_lists(self._h, samples_per_px, C.byref(on)), "rayz_hip_scene_get_primary_lists")
        return bool(on.value)

    def set_cell_lists(self, mode: int) -> None:
        """capi.CELL_LISTS_AUTO, _OFF or _ON: whether flat-list renders resolve a segment whose ray crosses the small spheres' slab
        under a handful of cells from those cells instead of a scan; the frame is the same either way."""
        capi.check(self._lib, self._lib.rayz_hip_scene_set_cell_lists(self._h, mode), "rayz_hip_scene_set_cell_lists")

    def uses_cell_lists(self) -> bool:
        """Whether a flat-list render would use the cells (what AUTO decides, if nothing was set; False for a scene without cells)."""
        on = C.c_uint32()
        capi.check(self._lib, self._lib.rayz_hip_scene_get_cell_lists(self._h, C.byref(on)), "rayz_hip_scene_get_cell_lists")
        return bool(on.value)

    # ---- ray queries (`findHit`, include/rayz_hip.h: rayz_hip_scene_query*) ----
    def query(self, rays, tmin: float = 1e-3, kind: str = "nearest", traversal: int = capi.TRAVERSAL_AUTO,
              outputs=QUERY_OUTPUTS, stream: int = 0) -> "QueryResult":
        """What each ray hits: `rays` is a torch tensor on the scene's device, (n, 8) {ox, oy, oz, time, dx, dy, dz, tmax},
        float32 or float64 (which selects the precision).  kind "nearest" fills the requested `outputs` (any of QUERY_OUTPUTS),
        "any" only `hit`.  Blocks for the bound check of the batch; the query itself is asynchronous on `stream` (0: the library's
        stream, after torch's work on the device has finished; another stream must itself be ordered after the rays' producer).
        The rays (their contiguous copy) and the outputs are kept alive by the scene until query_sync() or the next query."""
        import torch

        if not isinstance(rays, torch.Tensor) or not rays.is_cuda:
            raise ValueError("rays must be a torch tensor in GPU memory")
        if rays.device.index != self.device:
            raise ValueError(f"rays are on cuda:{rays.device.index}, the scene on cuda:{self.device}")
        if rays.dim() != 2 or rays.shape[1] != 8:
            raise ValueError(f"rays must be (n, 8), got {tuple(rays.shape)}")
        if rays.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"rays must be float32 or float64, got {rays.dtype}")
        if kind not in ("nearest", "any"):
            raise ValueError(f"kind must be 'nearest' or 'any', got {kind!r}")
        rays = rays.contiguous()
        n = rays.shape[0]
        if kind == "any":
            outputs = ("hit",)
        res = QueryResult._alloc((n,), rays.dtype, rays.device, outputs)
        self._query_prologue(stream)
        q = capi.QueryParams(n_rays=n, kind=capi.QUERY_ANY if kind == "any" else capi.QUERY_NEAREST,
                             precision=capi.PRECISION_F64 if rays.dtype == torch.float64 else capi.PRECISION_F32,
                             traversal=traversal, tmin=tmin)
        rc = self._lib.rayz_hip_scene_query(self._h, C.byref(q), C.c_void_p(rays.data_ptr() if n else None),
                                            C.byref(res._outputs()), C.c_void_p(stream or None))
        capi.check(self._lib, rc, "rayz_hip_scene_query")
        self._inflight = (rays, res)
        return res

    def gbuffer(self, camera: capi.CameraDesc, params: capi.RenderParams, outputs=QUERY_OUTPUTS,
                stream: int = 0, chain=False) -> "QueryResult":
        """The camera form: one lens-centre ray per pixel of `params`' shard (getRay(px, py, null)), results shaped
        (rows_in_shard, width, ...) on the scene's device.  Asynchronous on `stream`; the outputs are kept alive by the scene until
        query_sync() or the next query.
        `chain` True, or a dict of RayzChainParams' fields (max_depth, max_fuzz; unnamed ones take capi.CHAIN_DEFAULTS): the
        specular-chain G-buffer (`rayz_hip_scene_query_camera_chain`) — every pixel's ray is followed through
        mirror-like metals and glass, the requested `outputs` are the last segment's record (albedo multiplied by the chain's
        tint), and the result also carries key, depth and first_index and is marked `is_chain`.  Such a result guides
        `Denoiser.run` / `run_guided` (its keys are used by default); `Temporal` refuses it: reprojection needs the first-hit
        point, so a caller of both fills two G-buffers per frame."""
        import torch

        rows = shard_rows(params)
        dtype = torch.float64 if params.precision == capi.PRECISION_F64 else torch.float32
        dev = torch.device("cuda", self.device)
        res = QueryResult._alloc((rows, params.width), dtype, dev, outputs)
        if chain is False or chain is None:
            self._query_prologue(stream)
            rc = self._lib.rayz_hip_scene_query_camera(self._h, C.byref(camera), C.byref(params), C.byref(res._outputs()),
                                                       C.c_void_p(stream or None))
            capi.check(self._lib, rc, "rayz_hip_scene_query_camera")
            self._inflight = (None, res)
            return res
        if chain is not True and not isinstance(chain, dict):
            raise ValueError(f"chain must be False, True or a dict of {sorted(capi.CHAIN_DEFAULTS)}, got {chain!r}")
        prm = _params(capi.ChainParams, capi.CHAIN_DEFAULTS, {} if chain is True else chain, "chain")
        res.key = torch.empty((rows, params.width), dtype=torch.int32, device=dev)
        res.depth = torch.empty((rows, params.width), dtype=torch.uint8, device=dev)
        res.first_index = torch.empty((rows, params.width), dtype=torch.int32, device=dev)
        res.is_chain = True
        co = capi.ChainOutputs()
        if res.key.numel():
            co.key, co.depth, co.first_index = res.key.data_ptr(), res.depth.data_ptr(), res.first_index.data_ptr()
        self._query_prologue(stream)
        rc = self._lib.rayz_hip_scene_query_camera_chain(self._h, C.byref(camera), C.byref(params), C.byref(prm), C.byref(res._outputs()),
                                                         C.byref(co), C.c_void_p(stream or None))
        capi.check(self._lib, rc, "rayz_hip_scene_query_camera_chain")
        self._inflight = (None, res)
        return res

    def gbuffer_sampled(self, camera: capi.CameraDesc, params: capi.RenderParams, samples: int | None = None,
                        outputs=SAMPLED_OUTPUTS, stream: int = 0) -> "SampledResult":
        """The sampled G-buffer (`rayz_hip_scene_query_camera_sampled`): per pixel of `params`' shard the means
        of albedo, normal and t, and the hit count, over the camera segments of the render's own paths 0 .. samples-1 of that
        pixel — jittered over the pixel, the lens disk and the shutter by `params`' seed and samples_per_px, exactly as
        `render_into(camera, params, ...)` draws them.  `samples` None: all samples_per_px of them.  `outputs`: any of
        SAMPLED_OUTPUTS.  Results shaped (rows_in_shard, width[, 3]); asynchronous on `stream`; kept alive by the scene until
        query_sync() or the next query."""
        import torch

        outputs = tuple(outputs)
        for k in outputs:
            if k not in SAMPLED_OUTPUTS:
                raise ValueError(f"unknown sampled output {k!r}; choose from {SAMPLED_OUTPUTS}")
        if samples is not None and (isinstance(samples, bool) or not isinstance(samples, int) or samples < 1):
            raise ValueError(f"samples must be None or an int >= 1, got {samples!r}")
        rows = shard_rows(params)
        dtype = torch.float64 if params.precision == capi.PRECISION_F64 else torch.float32
        dev = torch.device("cuda", self.device)
        res = SampledResult()
        res.samples = int(samples if samples is not None else params.samples_per_px)
        so = capi.SampledOutputs()
        for k in outputs:
            shape = (rows, params.width) + ((3,) if k in ("albedo", "normal") else ())
            t = torch.empty(shape, dtype=torch.int32 if k == "hits" else dtype, device=dev)
            setattr(res, k, t)
            if t.numel():
                setattr(so, k, t.data_ptr())
        prm = capi.SampledParams(samples=0 if samples is None else samples)
        self._query_prologue(stream)
        rc = self._lib.rayz_hip_scene_query_camera_sampled(self._h, C.byref(camera), C.byref(params), C.byref(prm), C.byref(so),
                                                           C.c_void_p(stream or None))
        capi.check(self._lib, rc, "rayz_hip_scene_query_camera_sampled")
        self._inflight = (None, res)
        return res

    def pick(self, camera: capi.CameraDesc, params: capi.RenderParams, px: int, py: int) -> int:
        """The hittable under pixel (px, py) of the frame `params` describes (-1: background): the camera form on the one-row
        shard that holds row py (tile_rows 1, shard_count = height), so the ray is exactly that pixel's G-buffer ray.  Blocks."""
        if not (0 <= px < params.width and 0 <= py < params.height):
            raise ValueError(f"pixel ({px}, {py}) outside {params.width}x{params.height}")
        p = capi.RenderParams.from_buffer_copy(params)
        p.tile_rows, p.shard_count, p.shard_index = 1, params.height, py
        r = self.gbuffer(camera, p, outputs=("index",))
        self.query_sync()
        return int(r.index[0, px].item())

    def query_sync(self) -> capi.RenderStats:
        """Waits for the last query on the scene; its counters (rayz_hip_query_sync)."""
        st = capi.RenderStats()
        capi.check(self._lib, self._lib.rayz_hip_query_sync(self._h, C.byref(st)), "rayz_hip_query_sync")
        self._inflight = None
        return st


class Progressive(_Handle):
    """One frame rendered in passes (`rayz_hip_progressive_*`): every `step` adds whole chunks of the chunk schedule and may
    write the frame so far; the last one writes the one-shot frame bit for bit.  Close it before its scene."""

    _destroy = "rayz_hip_progressive_destroy"  # (waits for the last pass and the last evaluation)

    def __init__(self, scene: DeviceScene, camera: capi.CameraDesc, params: capi.RenderParams, track_noise: bool = False,
                 adaptive: bool = False, min_chunks: int | None = None):
        self._lib = scene._lib
        self._scene = scene  # (kept alive: the handle renders on it)
        self._h = C.c_void_p()
        self.f64 = params.precision == capi.PRECISION_F64
        self.shape = (shard_rows(params), params.width)  # of the handle's shard
        self._inflight = None  # the tensors of the last noise() / render_until(): kept alive until the next call or close()
        capi.check(self._lib, self._lib.rayz_hip_progressive_create(scene._h, C.byref(camera), C.byref(params),
                                                                    C.byref(self._h)), "rayz_hip_progressive_create")
        if track_noise:
            self.track_noise()
        if adaptive:
            self.set_adaptive(min_chunks)
        elif min_chunks is not None:
            raise ValueError("min_chunks belongs to adaptive=True")

    def track_noise(self) -> None:
        """`rayz_hip_progressive_track_noise`: keep the chunk sums' second moments (before the first step only)."""
        capi.check(self._lib, self._lib.rayz_hip_progressive_track_noise(self._h), "rayz_hip_progressive_track_noise")

    @staticmethod
    def _noise_params(rel_error, mean_floor) -> capi.NoiseParams:
        d = capi.NOISE_DEFAULTS
        return capi.NoiseParams(d["rel_error"] if rel_error is None else rel_error, d["mean_floor"] if mean_floor is None else mean_floor)

    def _stream_prologue(self, stream: int) -> None:
        _stream_prologue(stream, self._scene.device)

    def noise(self, rel_error: float | None = None, mean_floor: float | None = None, var: bool = False, rel2: bool = False,
              summary: bool = True, stream: int = 0):
        """The noise estimate of the samples done so far (`rayz_hip_progressive_noise`).  Returns
        (summary, var, rel2): a capi.NoiseSummary (None with summary=False: then nothing blocks) and, where asked for, float32 torch
        tensors shaped (rows_in_shard, width) on the scene's device — the variance of each pixel's mean (channels summed) and its
        squared relative error.  The tensors are written asynchronously on `stream` and kept alive by the handle until the next
        call.  With summary=True the call has waited for them.  With summary=False WAIT BEFORE READING THEM: `stats()` waits for
        the handle's last evaluation (or synchronise your own stream).  Torch's stream is not ordered after the
        write, so a `.cpu()` without that wait may read unwritten memory."""
        import torch

        dev = torch.device("cuda", self._scene.device)
        tv = torch.empty(self.shape, dtype=torch.float32, device=dev) if var else None
        tr = torch.empty(self.shape, dtype=torch.float32, device=dev) if rel2 else None
        self._stream_prologue(stream)
        prm = self._noise_params(rel_error, mean_floor)
        sm = capi.NoiseSummary() if summary else None
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None and t.numel() else None)  # noqa: E731
        rc = self._lib.rayz_hip_progressive_noise(self._h, C.byref(prm), ptr(tv), ptr(tr), C.byref(sm) if summary else None,
                                                  C.c_void_p(stream or None))
        capi.check(self._lib, rc, "rayz_hip_progressive_noise")
        self._inflight = (tv, tr)
        return sm, tv, tr

    def noise_rgb(self, stream: int = 0):
        """The variance of the pixel mean per channel (`rayz_hip_progressive_noise_rgb`): a float32 tensor (rows_in_shard, width, 3)
        on the scene's device, +inf before the second chunk — what `Denoiser.run_guided` takes as `var_rgb`.  Written asynchronously
        on `stream` and kept alive by the handle until the next call; WAIT BEFORE READING IT on the host, as for `noise(summary=False)`
        (`stats()` waits for it).  A `run_guided` on the same stream (0: the library's) is ordered behind it."""
        import torch

        v = torch.empty(self.shape + (3,), dtype=torch.float32, device=torch.device("cuda", self._scene.device))
        self._stream_prologue(stream)
        rc = self._lib.rayz_hip_progressive_noise_rgb(self._h, C.c_void_p(v.data_ptr() if v.numel() else None), C.c_void_p(stream or None))
        capi.check(self._lib, rc, "rayz_hip_progressive_noise_rgb")
        self._inflight = (v,)
        return v

    def noise_state(self, stream: int = 0):
        """The moment state (`rayz_hip_progressive_noise_state`): a float64 tensor (rows_in_shard, width, 4), {Q_r, Q_g, Q_b, 0}."""
        import torch

        q = torch.empty(self.shape + (4,), dtype=torch.float64, device=torch.device("cuda", self._scene.device))
        self._stream_prologue(stream)
        rc = self._lib.rayz_hip_progressive_noise_state(self._h, C.c_void_p(q.data_ptr() if q.numel() else None), C.c_void_p(stream or None))
        capi.check(self._lib, rc, "rayz_hip_progressive_noise_state")
        self._inflight = (q,)
        return q

    def render_until(self, rel_error: float | None = None, mean_floor: float | None = None, max_unconverged_fraction: float = 0.0,
                     min_samples_per_pass: int = 0, out=None, stream: int = 0) -> capi.NoiseSummary:
        """Render until converged (`rayz_hip_progressive_run_until`): passes of at least `min_samples_per_pass` samples until at most
        `max_unconverged_fraction` of the pixels are unconverged or the schedule ends (`done` tells which).  `out`: an optional
        torch tensor (rows_in_shard, width, 3) of the handle's precision on the scene's device that receives the frame it stopped
        at.  Blocks; returns the last summary."""
        self._check_out(out)
        self._stream_prologue(stream)
        prm = self._noise_params(rel_error, mean_floor)
        sm = capi.NoiseSummary()
        fn = self._lib.rayz_hip_progressive_run_until_f64 if self.f64 else self._lib.rayz_hip_progressive_run_until
        rc = fn(self._h, C.byref(prm), max_unconverged_fraction, min_samples_per_pass,
                C.c_void_p(out.data_ptr() if out is not None and out.numel() else None), C.byref(sm), C.c_void_p(stream or None))
        capi.check(self._lib, rc, "rayz_hip_progressive_run_until")
        self._inflight = (out,)
        return sm

    # ---- adaptive passes (`rayz_hip_progressive_set_adaptive` ..) ----
    def set_adaptive(self, min_chunks: int | None = None) -> None:
        """`rayz_hip_progressive_set_adaptive`: trace only unconverged pixels from now on (before the first step only)."""
        mc = capi.ADAPTIVE_DEFAULT_MIN_CHUNKS if min_chunks is None else int(min_chunks)
        capi.check(self._lib, self._lib.rayz_hip_progressive_set_adaptive(self._h, mc), "rayz_hip_progressive_set_adaptive")

    def _check_out(self, out):
        import torch

        if out is None:
            return
        want = torch.float64 if self.f64 else torch.float32
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.device.index != self._scene.device:
            raise ValueError(f"out must be a torch tensor on cuda:{self._scene.device}")
        if out.dtype != want or tuple(out.shape) != self.shape + (3,) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous {want} tensor shaped {self.shape + (3,)}")

    def _adaptive_call(self, name, rel_error, mean_floor, min_samples, out, stream) -> capi.AdaptiveSummary:
        self._check_out(out)
        self._stream_prologue(stream)
        prm = self._noise_params(rel_error, mean_floor)
        sm = capi.AdaptiveSummary()
        fn = getattr(self._lib, name + ("_f64" if self.f64 else ""))
        rc = fn(self._h, C.byref(prm), min_samples, C.c_void_p(out.data_ptr() if out is not None and out.numel() else None), C.byref(sm),
                C.c_void_p(stream or None))
        capi.check(self._lib, rc, name)
        self._inflight = (out,)
        return sm

    def adaptive_step(self, rel_error: float | None = None, mean_floor: float | None = None, min_samples: int = 0, out=None,
                      stream: int = 0) -> capi.AdaptiveSummary:
        """One adaptive pass (`rayz_hip_progressive_adaptive_step`): the window `step(min_samples)` would take, for the pixels
        still active; then every active pixel with rel2 <= rel_error^2 freezes.  `out`: an optional torch tensor (rows_in_shard,
        width, 3) of the handle's precision; pass the SAME tensor to every pass and it holds the whole frame after each (another
        tensor than the last pass's — and any tensor after a pass that got none — is written whole).  On a finished run nothing is traced and `out` receives the frame.
        Blocks; returns the summary (`active`: pixels the next pass traces)."""
        return self._adaptive_call("rayz_hip_progressive_adaptive_step", rel_error, mean_floor, min_samples, out, stream)

    def render_adaptive(self, rel_error: float | None = None, mean_floor: float | None = None, min_samples_per_pass: int = 0, out=None,
                        stream: int = 0) -> capi.AdaptiveSummary:
        """Adaptive passes until no pixel is active or the schedule ends (`rayz_hip_progressive_run_adaptive`); `out` receives the
        frame.  Blocks; returns the last summary (`samples_traced` against pixels x spp is the saving)."""
        return self._adaptive_call("rayz_hip_progressive_run_adaptive", rel_error, mean_floor, min_samples_per_pass, out, stream)

    def _adaptive_read(self, name, stream):
        import torch

        t = torch.empty(self.shape, dtype=torch.int32, device=torch.device("cuda", self._scene.device))  # (uint32 values < 2^31)
        self._stream_prologue(stream)
        rc = getattr(self._lib, name)(self._h, C.c_void_p(t.data_ptr() if t.numel() else None), C.c_void_p(stream or None))
        capi.check(self._lib, rc, name)
        return t

    def sample_counts(self, stream: int = 0):
        """N_i, the samples behind every pixel's value (`rayz_hip_progressive_sample_counts`): an int32 tensor (rows_in_shard,
        width) on the scene's device.  Blocks."""
        return self._adaptive_read("rayz_hip_progressive_sample_counts", stream)

    def frozen_at(self, stream: int = 0):
        """The chunk count at which every pixel froze, 0 for an active one (`rayz_hip_progressive_frozen_at`).  Blocks."""
        return self._adaptive_read("rayz_hip_progressive_frozen_at", stream)

    def step(self, min_samples: int = 0, out_ptr: int = 0, stream: int = 0) -> None:
        """One pass of at least `min_samples` samples per pixel (0: one chunk; 0xFFFFFFFF: the rest), asynchronous on `stream`;
        `out_ptr` (device memory, optional) receives the frame so far."""
        fn = self._lib.rayz_hip_progressive_step_f64 if self.f64 else self._lib.rayz_hip_progressive_step
        capi.check(self._lib, fn(self._h, min_samples, C.c_void_p(out_ptr or None), C.c_void_p(stream or None)),
                   "rayz_hip_progressive_step")

    def _info(self, total: bool = False):
        s, c, n = C.c_uint32(), C.c_uint32(), C.c_uint32()
        st = capi.RenderStats() if total else None
        capi.check(self._lib, self._lib.rayz_hip_progressive_info(self._h, C.byref(s), C.byref(c), C.byref(n),
                                                                  C.byref(st) if total else None),
                   "rayz_hip_progressive_info")
        return s.value, c.value, n.value, st

    @property
    def samples_done(self) -> int:
        return self._info()[0]

    @property
    def chunks_done(self) -> int:
        return self._info()[1]

    @property
    def n_chunks(self) -> int:
        return self._info()[2]

    @property
    def done(self) -> bool:
        _, c, n, _ = self._info()
        return c == n

    def stats(self) -> capi.RenderStats:
        """Counters summed over the passes so far (waits for them)."""
        return self._info(total=True)[3]


class Denoiser(_Handle):
    """A G-buffer-guided à-trous filter for whole float32 frames of one size (`rayz_hip_denoiser_*`):
    `run(frame, scene.gbuffer(camera, params))` returns the filtered frame; `run_guided(frame, progressive.noise_rgb(), gbuffer)`
    also weighs every pixel by its own noise estimate (§4.13).  `device` None: the default device of init()."""

    _destroy = "rayz_hip_denoiser_destroy"  # (waits for the handle's last run)

    def __init__(self, width: int, height: int, device: int | None = None):
        self._lib = capi.load()
        self._h = C.c_void_p()
        self.width, self.height = int(width), int(height)
        capi.check(self._lib, self._lib.rayz_hip_denoiser_create(-1 if device is None else device, self.width, self.height,
                                                                 C.byref(self._h)), "rayz_hip_denoiser_create")
        self._device = device if device is not None else _default_device
        self._inflight = None  # the tensors of the last run: kept alive until the next run or close() (the kernels may still use them)

    def _set_keys(self, gbuffer, keys):
        """The surface keys of a run (`rayz_hip_denoiser_set_keys`): `keys` "auto" — the gbuffer's `key` if it is a
        chain result, else none —, None for none, or a (height, width) int32 tensor on the handle's device.  Returns the tensor."""
        import torch

        if isinstance(keys, str):
            if keys != "auto":
                raise ValueError(f"keys must be 'auto', None or a tensor, got {keys!r}")
            keys = gbuffer.key if getattr(gbuffer, "is_chain", False) else None
        if keys is not None:
            _check_tensor("keys", keys, torch.int32, (self.height, self.width), self._device, "the denoiser")
        capi.check(self._lib, self._lib.rayz_hip_denoiser_set_keys(self._h, C.c_void_p(keys.data_ptr() if keys is not None else None)),
                   "rayz_hip_denoiser_set_keys")
        return keys

    def _checked(self, prm, inputs, gbuffer, out, var_out):
        """The tensor checks of a run, in argument order: the (name, tensor) `inputs`, the guides `prm.flags` asks for, `out` (None: a
        new tensor) and the optional `var_out`.  Returns (out, var_out or None, the guides' names)."""
        import torch

        frame = (self.height, self.width, 3)
        dev = torch.device("cuda", self._device)
        need = ["index", "normal", "point"] + (["albedo"] if prm.flags & capi.DENOISE_ALBEDO else [])
        if out is None:
            out = torch.empty(frame, dtype=torch.float32, device=dev)
        var_out = _optional_out(var_out, frame[:2], dev)
        _check_frame_tensors("the denoiser", self._device, frame, inputs, gbuffer, need, [("out", out, frame), ("var_out", var_out, frame[:2])])
        return out, var_out, need

    def run(self, rgb, gbuffer: "QueryResult", out=None, stream: int = 0, keys="auto", **params):
        """Filters `rgb` ((height, width, 3) float32 on the handle's device) guided by `gbuffer` (index, normal, point and — unless
        flags drops DENOISE_ALBEDO — albedo of a float32 camera query of the same frame) into `out` (default: a new tensor;
        `out=rgb` filters in place).  `params`: the fields of RayzDenoiseParams (levels, normal_power_log2, flags, sigma_color,
        sigma_plane); unnamed ones take capi.DENOISE_DEFAULTS.  `keys`: surface keys, (height, width) int32 — a tap whose key differs
        from the centre pixel's is skipped (§4.18); "auto" (the default) takes `gbuffer.key` when the gbuffer is a chain result and
        none otherwise, None switches them off.  Asynchronous on `stream` (0: the library's stream, after torch's
        work on the device has finished; another stream must itself be ordered after the inputs' producers)."""
        prm = _params(capi.DenoiseParams, capi.DENOISE_DEFAULTS, params, "denoise")
        out, _, need = self._checked(prm, [("rgb", rgb)], gbuffer, out, False)
        keys = self._set_keys(gbuffer, keys)
        _stream_prologue(stream, self._device)
        o = _gbuffer_pointers(gbuffer, need)
        rc = self._lib.rayz_hip_denoiser_run(self._h, C.byref(prm), C.c_void_p(rgb.data_ptr()), C.byref(o), C.c_void_p(out.data_ptr()),
                                             C.c_void_p(stream or None))
        capi.check(self._lib, rc, "rayz_hip_denoiser_run")
        self._inflight = (rgb, gbuffer, out, keys)
        return out

    def run_guided(self, rgb, var_rgb, gbuffer: "QueryResult", out=None, var_out=None, stream: int = 0, tap_level: int = 0, tap_out=None,
                   keys="auto", **params):
        """The variance-guided filter (`rayz_hip_denoiser_run_guided`): as `run`, with `var_rgb` — (height, width, 3)
        float32, the variance of each channel of `rgb`'s pixel means (`Progressive.noise_rgb()`) — steering the colour weight pixel
        by pixel.  `var_out`: True for a new (height, width) float32 tensor, or such a tensor, to receive the variance left in the
        demodulated colour; then the call returns (out, var_out).  `params`: the fields of RayzDenoiseGuidedParams (levels,
        normal_power_log2, flags, sigma_color — in standard deviations —, sigma_plane, var_floor); unnamed ones take
        capi.DENOISE_GUIDED_DEFAULTS.  `tap_level` t > 0 (`rayz_hip_denoiser_run_guided_tap`): the run also writes the re-modulated
        colour after t levels — what a run with levels=t returns — to `tap_out` (default: a new tensor; neither `rgb` nor `out`),
        which the call returns as a further value; t = 1 is what `Temporal.feedback` takes.  `keys`: as `run`."""
        import torch

        prm = _params(capi.DenoiseGuidedParams, capi.DENOISE_GUIDED_DEFAULTS, params, "denoise")
        out, var_out, need = self._checked(prm, [("rgb", rgb), ("var_rgb", var_rgb)], gbuffer, out, var_out)
        if tap_level:
            frame = (self.height, self.width, 3)
            if tap_out is None:
                tap_out = torch.empty(frame, dtype=torch.float32, device=torch.device("cuda", self._device))
            _check_tensor("tap_out", tap_out, torch.float32, frame, self._device, "the denoiser")
        elif tap_out is not None:
            raise ValueError("tap_out needs tap_level > 0")
        keys = self._set_keys(gbuffer, keys)
        _stream_prologue(stream, self._device)
        o = _gbuffer_pointers(gbuffer, need)
        if tap_level:
            rc = self._lib.rayz_hip_denoiser_run_guided_tap(self._h, C.byref(prm), C.c_void_p(rgb.data_ptr()), C.c_void_p(var_rgb.data_ptr()),
                                                            C.byref(o), C.c_void_p(out.data_ptr()),
                                                            C.c_void_p(var_out.data_ptr() if var_out is not None else None), int(tap_level),
                                                            C.c_void_p(tap_out.data_ptr()), C.c_void_p(stream or None))
            capi.check(self._lib, rc, "rayz_hip_denoiser_run_guided_tap")
            self._inflight = (rgb, var_rgb, gbuffer, out, var_out, tap_out, keys)
            return (out, tap_out) if var_out is None else (out, var_out, tap_out)
        rc = self._lib.rayz_hip_denoiser_run_guided(self._h, C.byref(prm), C.c_void_p(rgb.data_ptr()), C.c_void_p(var_rgb.data_ptr()),
                                                    C.byref(o), C.c_void_p(out.data_ptr()),
                                                    C.c_void_p(var_out.data_ptr() if var_out is not None else None), C.c_void_p(stream or None))
        capi.check(self._lib, rc, "rayz_hip_denoiser_run_guided")
        self._inflight = (rgb, var_rgb, gbuffer, out, var_out, keys)
        return out if var_out is None else (out, var_out)

    def timing(self):
        """Waits for the last run; its HIP-event times in ms: (pack pass, [level 0, level 1, ..]) (`rayz_hip_denoiser_timing`)."""
        n, ms = C.c_uint32(), (C.c_float * 9)()
        capi.check(self._lib, self._lib.rayz_hip_denoiser_timing(self._h, C.byref(n), ms, 9), "rayz_hip_denoiser_timing")
        return ms[0], [ms[1 + l] for l in range(n.value)]


# The order in which the f x f phases (px, py) of a lattice are visited: Bayer's ordered-dither matrices for 2 and 4 (every prefix
# of the sequence is spread as evenly over the block as that many points can be), a table in the same spirit for 3 (three
# diagonals, each a Latin pattern).  A parameter, not contract: any permutation of the phases rebuilds the frame.
_PHASE_ORDER = {
    2: ((0, 2),
        (3, 1)),
    3: ((0, 6, 3),
        (4, 1, 7),
        (8, 5, 2)),
    4: ((0, 8, 2, 10),
        (12, 4, 14, 6),
        (3, 11, 1, 9),
        (15, 7, 13, 5)),
}


def phase_sequence(f: int):
    """All f x f phases (px, py) of an every-f-th-pixel lattice, each once, in the order a still camera should cycle them."""
    if f not in _PHASE_ORDER:
        raise ValueError(f"lattice factor {f}: must be 2, 3 or 4")
    rank = _PHASE_ORDER[f]  # rank[py][px]: when that phase is visited
    return sorted(((px, py) for py in range(f) for px in range(f)), key=lambda p: rank[p[1]][p[0]])


def _check_phase(f: int, phase):
    px, py = (int(v) for v in phase)
    if f < 1 or not (0 <= px < f and 0 <= py < f):
        raise ValueError(f"phase {tuple(phase)} outside the {f}x{f} block")
    return px, py


def lattice_pixels(width: int, height: int, f: int, phase, order: str = "rows", device=None):
    """Every f-th pixel of an unsharded width x height frame, starting at `phase` = (px, py): the list `DeviceScene.render_pixels`
    takes, and where each entry belongs.  Returns (pixels, dest), int32 torch tensors on `device` (None: the CPU): pixels[k] =
    (f·j + py)·width + f·i + px for the lattice pixel (i, j), dest[k] = j·(width / f) + i, its row-major index in the
    (height / f, width / f) lattice frame.  `order` "rows" lists the lattice row by row; "tiles" deals it in 8x8 tiles of the
    lattice frame (tile rows first, a tile's pixels row by row), as whole frames are dealt to the waves.  Both list the same set."""
    import torch

    px, py = _check_phase(f, phase)
    if width <= 0 or height <= 0 or width % f or height % f:
        raise ValueError(f"frame {width}x{height}: not a positive multiple of the factor {f} in both directions")
    if order not in ("rows", "tiles"):
        raise ValueError(f"order must be 'rows' or 'tiles', got {order!r}")
    lw, lh = width // f, height // f
    j, i = np.divmod(np.arange(lw * lh, dtype=np.int64), lw)
    if order == "tiles":
        at = np.lexsort((i % 8, j % 8, i // 8, j // 8))  # (the last key sorts first)
        j, i = j[at], i[at]
    pixels = (f * j + py) * width + f * i + px
    dest = j * lw + i
    if pixels.size and pixels.max() >= 2 ** 31:
        raise ValueError(f"frame {width}x{height}: pixel indices beyond int32")
    as_t = lambda a: torch.from_numpy(a.astype(np.int32)).to(device if device is not None else "cpu")  # noqa: E731
    return as_t(pixels), as_t(dest)


def lattice_counts(width: int, height: int, f: int, phase, spp: int, device=None):
    """The sample counts of a lattice frame, for `Temporal.step` / `step_moments`: an int32 (height, width) torch
    tensor on `device` (None: the CPU) with `spp` at the pixels `lattice_pixels(width, height, f, phase)` lists and 0 elsewhere."""
    import torch

    px, py = _check_phase(f, phase)
    if width <= 0 or height <= 0 or width % f or height % f:
        raise ValueError(f"frame {width}x{height}: not a positive multiple of the factor {f} in both directions")
    if not 0 <= int(spp) <= 1 << 24:
        raise ValueError(f"spp {spp}: must lie in 0 .. 2^24 (it is used as f32)")
    counts = np.zeros((height, width), np.int32)
    counts[py::f, px::f] = int(spp)
    return torch.from_numpy(counts).to(device if device is not None else "cpu")


def lowres_camera(camera: capi.CameraDesc, factor: int) -> capi.CameraDesc:
    """The camera of a frame traced at 1/`factor` of the resolution in each direction: every low-resolution pixel sits at the centre
    of its factor x factor block of `camera`'s pixels.  `px_du` and `px_dv` are multiplied by the factor and
    `px_origin` — the centre of pixel (0, 0) — moves by ((factor - 1) / 2)·(px_du + px_dv); everything else is unchanged."""
    f = int(factor)
    if f < 1:
        raise ValueError(f"factor {factor}: must be a positive integer")
    cam = capi.CameraDesc.from_buffer_copy(camera)
    for k in range(3):
        cam.px_du[k] = camera.px_du[k] * f
        cam.px_dv[k] = camera.px_dv[k] * f
        cam.px_origin[k] = camera.px_origin[k] + 0.5 * (f - 1) * (camera.px_du[k] + camera.px_dv[k])
    return cam


def lowres_params(params: capi.RenderParams, factor: int) -> capi.RenderParams:
    """`params` for the frame `lowres_camera` looks at: width and height divided by the factor.  Raises unless both divide exactly,
    and on a shard other than the whole frame (rows of a shard are not image neighbours)."""
    f = int(factor)
    if f < 1:
        raise ValueError(f"factor {factor}: must be a positive integer")
    if params.width % f or params.height % f or not params.width or not params.height:
        raise ValueError(f"frame {params.width}x{params.height} is not a multiple of the factor {f} in both directions")
    if params.shard_count > 1 or params.shard_index:
        raise ValueError(f"shard {params.shard_index} of {params.shard_count}: a low-resolution frame is a whole frame")
    p = capi.RenderParams.from_buffer_copy(params)
    p.width, p.height = params.width // f, params.height // f
    return p


class Upscaler(_Handle):
    """Guided upscaling (`rayz_hip_upscaler_*`): rebuilds a `width` x `height` float32 frame from one traced at
    1/`factor` of the resolution in each direction (`lowres_camera`, `lowres_params`), under the full-size G-buffer.  `device` None:
    the default device of init()."""

    _destroy = "rayz_hip_upscaler_destroy"  # (waits for the handle's last run)

    def __init__(self, width: int, height: int, factor: int, device: int | None = None):
        self._lib = capi.load()
        self._h = C.c_void_p()
        self.width, self.height, self.factor = int(width), int(height), int(factor)
        capi.check(self._lib, self._lib.rayz_hip_upscaler_create(-1 if device is None else device, self.width, self.height, self.factor,
                                                                 C.byref(self._h)), "rayz_hip_upscaler_create")
        self._device = device if device is not None else _default_device
        self._inflight = None  # the tensors of the last run: kept alive until the next run or close() (the kernels may still use them)
        self._inflight_footprint = None  # .. and of the last footprint_albedo call

    def close(self) -> None:
        super().close()
        self._inflight_footprint = None

    def footprint_albedo(self, gbuffer_lo: "QueryResult", gbuffer_hi: "QueryResult", out=None, count=False, stream: int = 0):
        """The albedo a frame of block means should be demodulated by (`rayz_hip_upscaler_footprint_albedo`): for
        every low-resolution pixel the mean of the full-size albedos of its factor x factor block that lie on its own surface (the
        same `index`), (1, 1, 1) for a background pixel, `gbuffer_lo.albedo` itself where no pixel of the block is on that surface.
        `gbuffer_lo`, `gbuffer_hi`: float32 camera queries of the low-resolution and of the full frame; index and albedo are read.
        Returns `out` (default: a new (height / factor, width / factor, 3) float32 tensor; never `gbuffer_lo.albedo` itself).
        `count` True, or a (height / factor, width / factor) uint8 tensor: the number of pixels averaged is returned as a further
        value.  Asynchronous on `stream`, as `run`, and ordered with the handle's runs."""
        import torch

        hi = (self.height, self.width, 3)
        lo = (self.height // self.factor, self.width // self.factor, 3)
        dev = torch.device("cuda", self._device)
        need = ["index", "albedo"]
        if out is None:
            out = torch.empty(lo, dtype=torch.float32, device=dev)
        if count is True:
            count = torch.empty(lo[:2], dtype=torch.uint8, device=dev)
        elif count is False:
            count = None
        tensors = []
        for name, g, frame in (("gbuffer_lo", gbuffer_lo, lo), ("gbuffer_hi", gbuffer_hi, hi)):
            tensors += [(f"{name}.{k}", getattr(g, k), torch.int32 if k == "index" else torch.float32, frame[:2] if k == "index" else frame)
                        for k in need]
        tensors.append(("out", out, torch.float32, lo))
        if count is not None:
            tensors.append(("count", count, torch.uint8, lo[:2]))
        for t in tensors:
            _check_tensor(*t, self._device, "the upscaler")
        _stream_prologue(stream, self._device)
        rc = self._lib.rayz_hip_upscaler_footprint_albedo(self._h, C.byref(_gbuffer_pointers(gbuffer_lo, need)),
                                                          C.byref(_gbuffer_pointers(gbuffer_hi, need)), C.c_void_p(out.data_ptr()),
                                                          C.c_void_p(count.data_ptr() if count is not None else None), C.c_void_p(stream or None))
        capi.check(self._lib, rc, "rayz_hip_upscaler_footprint_albedo")
        self._inflight_footprint = (gbuffer_lo, gbuffer_hi, out, count)
        return out if count is None else (out, count)

    def footprint_timing(self) -> float:
        """Waits for the last `footprint_albedo` call; its launch's HIP-event time in ms (`rayz_hip_upscaler_footprint_timing`)."""
        ms = C.c_float()
        capi.check(self._lib, self._lib.rayz_hip_upscaler_footprint_timing(self._h, C.byref(ms)), "rayz_hip_upscaler_footprint_timing")
        return ms.value

    def run(self, rgb_lo, gbuffer_lo: "QueryResult", gbuffer_hi: "QueryResult", var_rgb=None, out=None, var_out=None, stage=False,
            stream: int = 0, phase=None, footprint=False, **params):
        """`rgb_lo`: (height / factor, width / factor, 3) float32 on the handle's device; `gbuffer_lo`, `gbuffer_hi`: float32 camera
        queries of the low-resolution and of the full frame (index, normal, point, and albedo with flags=DENOISE_ALBEDO).  Returns `out` (default: a new (height, width, 3) tensor).  With `var_rgb` — the per-channel variance of `rgb_lo`'s
        pixel means, shaped as it — the call returns (out, var): the per-channel MARGINAL variance of every full pixel (`var_out`: a
        tensor to receive it).  `stage` True, or a (height, width) uint8 tensor: the stage map (0, 1, 2) is returned as a further
        value.  `params`: normal_power_log2, flags, form, sigma_plane of RayzUpscaleParams; unnamed ones take capi.UPSCALE_DEFAULTS —
        flags 0: demodulating by the low-resolution albedo measured far worse than not doing it.
        `phase` (px, py): `rgb_lo` is a LATTICE frame (`lattice_pixels`, `DeviceScene.render_pixels`) whose pixel (i, j) is full
        pixel (factor·i + px, factor·j + py), and `gbuffer_lo` is `gbuffer_hi.lattice(factor, phase)`
        (`rayz_hip_upscaler_run_phase`): the sampled pixels come back as they are, the others are rebuilt around them.  None: the
        frame of block means a `lowres_camera` traces.
        `footprint` True (needs flags=DENOISE_ALBEDO, and no `phase`: a lattice sample is a real pixel with its own albedo): the
        low-resolution frame is demodulated by `footprint_albedo(gbuffer_lo, gbuffer_hi)` instead of `gbuffer_lo.albedo` (§4.24),
        computed on the same stream; `gbuffer_lo` itself is not modified.
        No output may share memory with an input.  Asynchronous on `stream`, as `Denoiser.run`."""
        import torch

        prm = _params(capi.UpscaleParams, capi.UPSCALE_DEFAULTS, params, "upscale")
        prm.factor = self.factor
        if phase is not None:
            phase = _check_phase(self.factor, phase)
        if footprint:
            if phase is not None:
                raise ValueError("footprint=True with phase=: a lattice sample is a real pixel with its own albedo")
            if not prm.flags & capi.DENOISE_ALBEDO:
                raise ValueError("footprint=True needs flags=DENOISE_ALBEDO: without it nothing is demodulated")
        hi = (self.height, self.width, 3)
        lo = (self.height // self.factor, self.width // self.factor, 3)
        dev = torch.device("cuda", self._device)
        need = ["index", "normal", "point"] + (["albedo"] if prm.flags & capi.DENOISE_ALBEDO else [])
        if out is None:
            out = torch.empty(hi, dtype=torch.float32, device=dev)
        if var_out is not None and var_rgb is None:
            raise ValueError("var_out needs var_rgb")
        if var_rgb is not None and var_out is None:
            var_out = torch.empty(hi, dtype=torch.float32, device=dev)
        if stage is True:
            stage = torch.empty(hi[:2], dtype=torch.uint8, device=dev)
        elif stage is False:
            stage = None
        tensors = [("rgb_lo", rgb_lo, torch.float32, lo)]
        if var_rgb is not None:
            tensors.append(("var_rgb", var_rgb, torch.float32, lo))
        for name, g, frame in (("gbuffer_lo", gbuffer_lo, lo), ("gbuffer_hi", gbuffer_hi, hi)):
            tensors += [(f"{name}.{k}", getattr(g, k), torch.int32 if k == "index" else torch.float32, frame[:2] if k == "index" else frame)
                        for k in need]
        tensors.append(("out", out, torch.float32, hi))
        if var_out is not None:
            tensors.append(("var_out", var_out, torch.float32, hi))
        if stage is not None:
            tensors.append(("stage", stage, torch.uint8, hi[:2]))
        for t in tensors:
            _check_tensor(*t, self._device, "the upscaler")
        given_lo = gbuffer_lo
        if footprint:
            gbuffer_lo = copy.copy(given_lo)  # (shallow: the caller's G-buffer keeps its albedo)
            gbuffer_lo.albedo = self.footprint_albedo(given_lo, gbuffer_hi, stream=stream)  # (its prologue is the run's)
        else:
            _stream_prologue(stream, self._device)
        args = (C.c_void_p(rgb_lo.data_ptr()), C.c_void_p(var_rgb.data_ptr() if var_rgb is not None else None),
                C.byref(_gbuffer_pointers(gbuffer_lo, need)), C.byref(_gbuffer_pointers(gbuffer_hi, need)),
                C.c_void_p(out.data_ptr()), C.c_void_p(var_out.data_ptr() if var_out is not None else None),
                C.c_void_p(stage.data_ptr() if stage is not None else None), C.c_void_p(stream or None))
        if phase is None:
            rc = self._lib.rayz_hip_upscaler_run(self._h, C.byref(prm), *args)
        else:
            rc = self._lib.rayz_hip_upscaler_run_phase(self._h, C.byref(prm), phase[0], phase[1], *args)
        capi.check(self._lib, rc, "rayz_hip_upscaler_run")
        self._inflight = (rgb_lo, var_rgb, given_lo, gbuffer_lo, gbuffer_hi, out, var_out, stage)
        res = (out,) + ((var_out,) if var_out is not None else ()) + ((stage,) if stage is not None else ())
        return res[0] if len(res) == 1 else res

    def timing(self):
        """Waits for the last run; its HIP-event times in ms: (pack launches, reconstruction launch) (`rayz_hip_upscaler_timing`)."""
        pack, up = C.c_float(), C.c_float()
        capi.check(self._lib, self._lib.rayz_hip_upscaler_timing(self._h, C.byref(pack), C.byref(up)), "rayz_hip_upscaler_timing")
        return pack.value, up.value


class Temporal(_Handle):
    """Temporal accumulation for whole float32 frames of one size (`rayz_hip_temporal_*`): every `step` blends
    the frame it is given into the history reprojected from the previous step's camera and returns the accumulated frame and its
    per-channel variance — what `Denoiser.run_guided` takes.  `device` None: the default device of init().  `moments` True: the
    handle is put into moments mode (`track_moments`, §4.16) and takes `step_moments`, which needs no variance input; with
    `feedback` True as well it also tracks feedback (`track_feedback`, §4.17) and takes `feedback`.  `resampling` "cubic": moving
    steps fetch the colour history with the 4x4 Catmull-Rom kernel where all sixteen history pixels are the same surface, and
    bilinearly elsewhere (`set_resampling`, §4.26); the default "bilinear" is §4.15 as it is.  `background` "accumulate": pixels
    whose centre ray misses the scene gather history too, reprojected by the view's turn alone (`set_background`, §4.27); the
    default "input" passes them through.  `clip` "variance": a moving step clamps the history's colour to mean ± `clip_gamma` sample
    deviations of the current frame's 7x7 neighbourhood on the same surface before it blends (`set_clip`, §4.28; `clip_gamma` and
    `clip_min_taps` None: capi.TEMPORAL_CLIP_DEFAULTS); the default "off" compares no colours."""

    _destroy = "rayz_hip_temporal_destroy"  # (waits for the handle's last step)

    def __init__(self, width: int, height: int, device: int | None = None, moments: bool = False, feedback: bool = False,
                 resampling: str = "bilinear", background: str = "input", clip: str = "off", clip_gamma: float | None = None,
                 clip_min_taps: float | None = None):
        self._lib = capi.load()
        self._h = C.c_void_p()
        self.width, self.height = int(width), int(height)
        capi.check(self._lib, self._lib.rayz_hip_temporal_create(-1 if device is None else device, self.width, self.height,
                                                                 C.byref(self._h)), "rayz_hip_temporal_create")
        self._device = device if device is not None else _default_device
        self._inflight = None  # the tensors of the last step: kept alive until the next step or close() (the kernel may still use them)
        self._taken = None  # the uint8 (height, width) tensor the library writes at every step (set_resampling), or None
        self._clipped = None  # .. and the one of set_clip
        self._clip_mode = "off"  # what set_clip last set: what `_counts` looks at (the library refuses such a step itself)
        if feedback and not moments:
            self.close()
            raise ValueError("feedback=True needs moments=True: only a moments handle tracks feedback")
        try:
            if resampling not in capi.TEMPORAL_RESAMPLING:
                raise ValueError(f"resampling must be one of {sorted(capi.TEMPORAL_RESAMPLING)}, got {resampling!r}")
            if feedback and resampling == "cubic":
                raise ValueError('feedback=True with resampling="cubic": a handle that tracks feedback has no cubic mode')
            if background not in capi.TEMPORAL_BACKGROUND:
                raise ValueError(f"background must be one of {sorted(capi.TEMPORAL_BACKGROUND)}, got {background!r}")
            if background == "accumulate" and (feedback or resampling == "cubic"):
                raise ValueError('background="accumulate" with feedback=True or resampling="cubic": neither accumulates the background')
            if moments:
                self.track_moments()
                if feedback:
                    self.track_feedback()
            if resampling != "bilinear":
                self.set_resampling(resampling)
            if background != "input":
                self.set_background(background)
            if clip not in capi.TEMPORAL_CLIP:
                raise ValueError(f"clip must be one of {sorted(capi.TEMPORAL_CLIP)}, got {clip!r}")
            if clip != "off" or clip_gamma is not None or clip_min_taps is not None:
                self.set_clip(clip, clip_gamma, clip_min_taps)
        except Exception:
            self.close()
            raise

    def track_moments(self) -> None:
        """Puts the handle into moments mode (`rayz_hip_temporal_track_moments`): only while it has no history — after creation
        or after `reset` —; a second call does nothing.  From then on the handle takes `step_moments` and refuses `step`."""
        capi.check(self._lib, self._lib.rayz_hip_temporal_track_moments(self._h), "rayz_hip_temporal_track_moments")

    def track_feedback(self) -> None:
        """Makes a moments handle keep the raw first moment beside its colour (`rayz_hip_temporal_track_feedback`): only while it
        has no history; a second call does nothing.  From then on `step_moments` takes its variance from that moment, and the
        handle takes `feedback`."""
        capi.check(self._lib, self._lib.rayz_hip_temporal_track_feedback(self._h), "rayz_hip_temporal_track_feedback")

    def set_resampling(self, resampling: str, taken=False) -> None:
        """How moving steps fetch the colour history from now on (`rayz_hip_temporal_set_resampling`): "bilinear"
        (the default, §4.15 as it is) or "cubic" — the clamped 4x4 Catmull-Rom kernel where all sixteen history pixels are the
        same surface, bilinear elsewhere.  May be changed between any two steps.  `taken`: True for a new uint8 (height, width)
        tensor, or the caller's, which every later step fills with 1 where the pixel took the sixteen taps and 0 elsewhere
        (`Temporal.taken`); False for none.  Limits: a handle that tracks feedback has no cubic mode, and a cubic handle takes no
        counts tensor as `spp`."""
        import torch

        if resampling not in capi.TEMPORAL_RESAMPLING:
            raise ValueError(f"resampling must be one of {sorted(capi.TEMPORAL_RESAMPLING)}, got {resampling!r}")
        if taken is True:
            taken = torch.empty((self.height, self.width), dtype=torch.uint8, device=torch.device("cuda", self._device))
        elif taken is False or taken is None:
            taken = None
        else:
            _check_tensor("taken", taken, torch.uint8, (self.height, self.width), self._device, "the temporal handle")
        capi.check(self._lib, self._lib.rayz_hip_temporal_set_resampling(self._h, capi.TEMPORAL_RESAMPLING[resampling],
                                                                         C.c_void_p(taken.data_ptr() if taken is not None else None)),
                   "rayz_hip_temporal_set_resampling")
        self._taken = taken  # (every later step writes it and keeps it in _inflight, so a step still running when it is replaced holds it)

    @property
    def resampling(self) -> str:
        """"bilinear" or "cubic": the handle's mode (`rayz_hip_temporal_get_resampling`)."""
        mode = C.c_uint32()
        capi.check(self._lib, self._lib.rayz_hip_temporal_get_resampling(self._h, C.byref(mode)), "rayz_hip_temporal_get_resampling")
        return {v: k for k, v in capi.TEMPORAL_RESAMPLING.items()}[mode.value]

    def set_background(self, background: str) -> None:
        """What steps do from now on with a pixel whose centre ray misses the scene (`rayz_hip_temporal_set_background`, DESIGN.md
        §4.27): "input" (the default) passes its input through; "accumulate" reprojects it by the turn of the view alone — the sky
        has no parallax — and blends it into the history of the previous frame's background pixels, in all four kinds of step; in
        a counts step a background pixel without samples keeps its history.  May be changed between any two steps.  Limits: a
        handle that tracks feedback or is in "cubic" resampling mode does not accumulate the background."""
        if background not in capi.TEMPORAL_BACKGROUND:
            raise ValueError(f"background must be one of {sorted(capi.TEMPORAL_BACKGROUND)}, got {background!r}")
        capi.check(self._lib, self._lib.rayz_hip_temporal_set_background(self._h, capi.TEMPORAL_BACKGROUND[background]),
                   "rayz_hip_temporal_set_background")

    @property
    def background(self) -> str:
        """"input" or "accumulate": the handle's background mode (`rayz_hip_temporal_get_background`)."""
        mode = C.c_uint32()
        capi.check(self._lib, self._lib.rayz_hip_temporal_get_background(self._h, C.byref(mode)), "rayz_hip_temporal_get_background")
        return {v: k for k, v in capi.TEMPORAL_BACKGROUND.items()}[mode.value]

    def set_clip(self, clip: str, gamma: float | None = None, min_taps: float | None = None, clipped=False) -> None:
        """Whether moving steps clip the colour history from now on (`rayz_hip_temporal_set_clip`): "off", or
        "variance" — a pixel that found history clamps its history's colour, per channel, to mean ± `gamma` sample deviations of
        the current frame over its 7x7 neighbourhood on the same surface (for a background pixel of an "accumulate" handle: over
        the neighbourhood's misses), where that has at least `min_taps` pixels; a moments handle moves the second moment with it.
        Static steps, first frames and pixels without history are unchanged.  `gamma` >= 0 (inf never clips) and `min_taps` in
        [2, 49]; None: capi.TEMPORAL_CLIP_DEFAULTS.  May be changed between any two steps.  `clipped`: True for a new uint8
        (height, width) tensor on the handle's device that every later step writes — 1 where the clip changed a channel of the
        pixel's colour history — or such a tensor (`Temporal.clipped`); False for none.  Limits: a handle that tracks feedback or
        is in "cubic" resampling mode has no clip mode, and a "variance" handle takes no counts tensor as spp."""
        import torch

        if clip not in capi.TEMPORAL_CLIP:
            raise ValueError(f"clip must be one of {sorted(capi.TEMPORAL_CLIP)}, got {clip!r}")
        prm = capi.TemporalClipParams(capi.TEMPORAL_CLIP_DEFAULTS["gamma"] if gamma is None else float(gamma),
                                      capi.TEMPORAL_CLIP_DEFAULTS["min_taps"] if min_taps is None else float(min_taps))
        if clipped is True:
            clipped = torch.empty((self.height, self.width), dtype=torch.uint8, device=torch.device("cuda", self._device))
        elif clipped is False or clipped is None:
            clipped = None
        else:
            _check_tensor("clipped", clipped, torch.uint8, (self.height, self.width), self._device, "the temporal handle")
        capi.check(self._lib, self._lib.rayz_hip_temporal_set_clip(self._h, capi.TEMPORAL_CLIP[clip], C.byref(prm),
                                                                   C.c_void_p(clipped.data_ptr() if clipped is not None else None)),
                   "rayz_hip_temporal_set_clip")
        self._clip_mode = clip
        self._clipped = clipped  # (every later step writes it and keeps it in _inflight, as the taken bytes)

    def _get_clip(self):
        mode, prm = C.c_uint32(), capi.TemporalClipParams()
        capi.check(self._lib, self._lib.rayz_hip_temporal_get_clip(self._h, C.byref(mode), C.byref(prm)), "rayz_hip_temporal_get_clip")
        return mode.value, prm

    @property
    def clip(self) -> str:
        """"off" or "variance": the handle's clip mode (`rayz_hip_temporal_get_clip`)."""
        mode, _ = self._get_clip()
        return next(k for k, v in capi.TEMPORAL_CLIP.items() if v == mode)

    @property
    def clip_params(self) -> dict:
        """{"gamma": .., "min_taps": ..}: the clip's parameters as the handle holds them (`rayz_hip_temporal_get_clip`)."""
        _, prm = self._get_clip()
        return {"gamma": prm.gamma, "min_taps": prm.min_taps}

    @property
    def clipped(self):
        """The uint8 (height, width) tensor `set_clip(..., clipped=...)` named, holding the last step's bytes once that step has
        finished: 1 where the clip changed a channel of the pixel's colour history.  None: no such tensor."""
        return self._clipped

    @property
    def taken(self):
        """The uint8 (height, width) tensor `set_resampling(..., taken=...)` named, holding the last step's bytes once that step has
        finished: 1 where the pixel's colour history came from the sixteen taps.  None: no such tensor."""
        return self._taken

    def feedback(self, rgb, stream: int = 0) -> None:
        """Replaces the colour history the last step left with `rgb` ((height, width, 3) float32 on the handle's device) — SVGF's
        feedback, `rgb` being `Denoiser.run_guided(..., tap_level=1)`'s tap (`rayz_hip_temporal_feedback`).  The
        history length and the moments stay; a pixel of `rgb` that is not finite keeps its colour.  Asynchronous on `stream`, as
        `step`."""
        import torch

        _check_tensor("rgb", rgb, torch.float32, (self.height, self.width, 3), self._device, "the temporal handle")
        _stream_prologue(stream, self._device)
        capi.check(self._lib, self._lib.rayz_hip_temporal_feedback(self._h, C.c_void_p(rgb.data_ptr()), C.c_void_p(stream or None)),
                   "rayz_hip_temporal_feedback")
        self._inflight = (self._inflight, rgb)  # (beside the last step's tensors, which the step's kernel may still use)

    def _step_prologue(self, inputs, gbuffer, out, var_out, planes, stream):
        """What both kinds of step do before their call: `out` and `var_out` (None: new tensors), the optional (height, width)
        outputs `planes` ((name, False / True / tensor) each), the tensor checks in argument order, the stream's prologue.  Returns
        (out, var_out, [a plane's tensor or None, ..], the guides' pointers)."""
        import torch

        if getattr(gbuffer, "is_chain", False):
            raise ValueError("the temporal handle needs a first-hit G-buffer (reprojection projects the first-hit point): this one is a "
                             "chain result; fill a second G-buffer without chain= for the temporal step")
        frame = (self.height, self.width, 3)
        dev = torch.device("cuda", self._device)
        need = ["index", "normal", "point"]
        if out is None:
            out = torch.empty(frame, dtype=torch.float32, device=dev)
        if var_out is None:
            var_out = torch.empty(frame, dtype=torch.float32, device=dev)
        planes = [(name, _optional_out(t, frame[:2], dev)) for name, t in planes]
        _check_frame_tensors("the temporal handle", self._device, frame, inputs, gbuffer, need,
                             [("out", out, frame), ("var_out", var_out, frame)] + [(name, t, frame[:2]) for name, t in planes])
        _stream_prologue(stream, self._device)
        return out, var_out, [t for _, t in planes], _gbuffer_pointers(gbuffer, need)

    def _counts(self, spp):
        """`spp` of a step: None for an int (the scalar step), or the checked int32 (height, width) tensor of per-pixel sample counts
        a counts step takes, which the library reads as uint32: no value may be negative."""
        import torch

        if not isinstance(spp, torch.Tensor):
            return None
        if self.resampling == "cubic":
            raise ValueError('a handle in "cubic" resampling mode takes no counts tensor as spp (set_resampling("bilinear") first)')
        if self._clip_mode == "variance":
            raise ValueError('a handle in "variance" clip mode takes no counts tensor as spp (set_clip("off") first)')
        _check_tensor("spp", spp, torch.int32, (self.height, self.width), self._device, "the temporal handle")
        if int(spp.min()) < 0:
            raise ValueError("spp holds a negative sample count")
        return spp

    def step(self, rgb, var_rgb, gbuffer: "QueryResult", camera: capi.CameraDesc, spp, out=None, var_out=None, length=False,
             stream: int = 0, **params):
        """One frame: `rgb` and `var_rgb` ((height, width, 3) float32 on the handle's device: the frame and the variance of each
        channel of its pixel means, `Progressive.noise_rgb()`), `gbuffer` (index, normal, point of a float32 camera query of the same
        frame), the `camera` both were made with and the frame's samples per pixel.  Returns (out, var_out) — new tensors by
        default; `out=rgb` / `var_out=var_rgb` step in place — and, with `length` True or a (height, width) float32 tensor, the
        history length in samples as a third value.  `params`: the fields of RayzTemporalParams (alpha_min, n_max, normal_cos_min,
        max_rel_dist); unnamed ones take capi.TEMPORAL_DEFAULTS.  Asynchronous on `stream` (0: the library's stream, after torch's
        work on the device has finished; another stream must itself be ordered after the inputs' producers).
        `spp` may instead be an int32 (height, width) tensor on the handle's device, values >= 0 — the samples this frame adds to
        each pixel (`lattice_counts`, `Progressive.sample_counts()`): the counts step (`rayz_hip_temporal_step_counts`, §4.23), in
        which a pixel with count 0 keeps its history whatever `rgb` and `var_rgb` hold there."""
        prm = _params(capi.TemporalParams, capi.TEMPORAL_DEFAULTS, params, "temporal")
        counts = self._counts(spp)
        out, var_out, (length,), o = self._step_prologue([("rgb", rgb), ("var_rgb", var_rgb)], gbuffer, out, var_out, [("length", length)],
                                                         stream)
        name = "rayz_hip_temporal_step" if counts is None else "rayz_hip_temporal_step_counts"
        rc = getattr(self._lib, name)(self._h, C.byref(prm), C.byref(camera), int(spp) if counts is None else C.c_void_p(counts.data_ptr()),
                                      C.c_void_p(rgb.data_ptr()), C.c_void_p(var_rgb.data_ptr()), C.byref(o), C.c_void_p(out.data_ptr()),
                                      C.c_void_p(var_out.data_ptr()), C.c_void_p(length.data_ptr() if length is not None else None),
                                      C.c_void_p(stream or None))
        capi.check(self._lib, rc, name)
        self._inflight = (rgb, var_rgb, gbuffer, out, var_out, length, counts, self._taken, self._clipped)  # (the step writes the taken and clipped bytes too)
        return (out, var_out) if length is None else (out, var_out, length)

    def step_moments(self, rgb, gbuffer: "QueryResult", camera: capi.CameraDesc, spp, out=None, var_out=None, length=False,
                     w2=False, stream: int = 0, **params):
        """One frame of a handle in moments mode (`rayz_hip_temporal_step_moments`): as `step` without `var_rgb` —
        the variance of the accumulated mean comes from the history's second moment, or where the history is too short from the
        frame's 7x7 neighbourhood on the same surface, so `rgb` may be a one-chunk frame from any source.  Returns (out, var_out)
        — new tensors by default; `out` must not be `rgb`: neighbours read the current frame — then, with `length` True or a
        (height, width) float32 tensor, the history length in samples, then, with `w2` likewise, W2 (the sum of the squared weights
        of the frames in `out`; 1 / W2 is the effective frame count).  `params`: the fields of RayzTemporalParams and of
        RayzTemporalMomentsParams (w2_max, min_taps); unnamed ones take capi.TEMPORAL_DEFAULTS and
        capi.TEMPORAL_MOMENTS_DEFAULTS.  Asynchronous on `stream`, as `step`.  `spp` may be a tensor of per-pixel sample counts as
        in `step` (`rayz_hip_temporal_step_moments_counts`, §4.23): a pixel with count 0 keeps its history and is left out of its
        neighbours' 7x7 estimates; a handle that tracks feedback refuses it."""
        import torch

        unknown = set(params) - set(capi.TEMPORAL_DEFAULTS) - set(capi.TEMPORAL_MOMENTS_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown temporal parameter(s) {sorted(unknown)}; choose from "
                             f"{sorted({**capi.TEMPORAL_DEFAULTS, **capi.TEMPORAL_MOMENTS_DEFAULTS})}")
        prm = _params(capi.TemporalParams, capi.TEMPORAL_DEFAULTS, {k: v for k, v in params.items() if k in capi.TEMPORAL_DEFAULTS},
                      "temporal")
        mprm = _params(capi.TemporalMomentsParams, capi.TEMPORAL_MOMENTS_DEFAULTS,
                       {k: v for k, v in params.items() if k in capi.TEMPORAL_MOMENTS_DEFAULTS}, "temporal")
        if out is rgb or (isinstance(out, torch.Tensor) and isinstance(rgb, torch.Tensor) and out.data_ptr() == rgb.data_ptr()):
            raise ValueError("out must not be rgb: a moments step cannot run in place (neighbours read the current frame)")
        counts = self._counts(spp)
        out, var_out, (length, w2), o = self._step_prologue([("rgb", rgb)], gbuffer, out, var_out, [("length", length), ("w2", w2)], stream)
        name = "rayz_hip_temporal_step_moments" if counts is None else "rayz_hip_temporal_step_moments_counts"
        rc = getattr(self._lib, name)(self._h, C.byref(prm), C.byref(mprm), C.byref(camera),
                                      int(spp) if counts is None else C.c_void_p(counts.data_ptr()), C.c_void_p(rgb.data_ptr()), C.byref(o),
                                      C.c_void_p(out.data_ptr()), C.c_void_p(var_out.data_ptr()),
                                      C.c_void_p(length.data_ptr() if length is not None else None),
                                      C.c_void_p(w2.data_ptr() if w2 is not None else None), C.c_void_p(stream or None))
        capi.check(self._lib, rc, name)
        self._inflight = (rgb, gbuffer, out, var_out, length, w2, counts, self._taken, self._clipped)
        return (out, var_out) + tuple(t for t in (length, w2) if t is not None)

    def reset(self) -> None:
        """Forgets the history: the next step is a first frame (`rayz_hip_temporal_reset`)."""
        capi.check(self._lib, self._lib.rayz_hip_temporal_reset(self._h), "rayz_hip_temporal_reset")

    def timing(self) -> float:
        """Waits for the last step; its HIP-event time in ms (`rayz_hip_temporal_timing`)."""
        ms = C.c_float()
        capi.check(self._lib, self._lib.rayz_hip_temporal_timing(self._h, C.byref(ms)), "rayz_hip_temporal_timing")
        return ms.value


class MultiScene(_Handle):
    """The pool replicated on several GPUs of the node (`rayz_hip_multi_create`): one call renders the whole frame —
    rows dealt to the devices in interleaved tiles, one RCCL gather (or peer copies) to devices[0], host output."""

    _destroy = "rayz_hip_multi_destroy"

    def __init__(self, scene: capi.SceneDesc, devices, transport: int = capi.GATHER_RCCL):
        self._lib = capi.load()
        self._h = C.c_void_p()
        self.devices = list(devices)
        arr = (C.c_int * len(self.devices))(*self.devices)
        capi.check(self._lib, self._lib.rayz_hip_multi_create(arr, len(self.devices), C.byref(scene), transport,
                                                              C.byref(self._h)), "rayz_hip_multi_create")

    def info(self):
        n, tr, ver = C.c_int(), C.c_uint32(), C.c_int()
        capi.check(self._lib, self._lib.rayz_hip_multi_info(self._h, C.byref(n), C.byref(tr), C.byref(ver)),
                   "rayz_hip_multi_info")
        return {"n_devices": n.value, "transport": tr.value, "rccl_version": ver.value}

    def render(self, camera: capi.CameraDesc, params: capi.RenderParams, u8: bool = False):
        """Returns (frame (h, w, 3), stats); `u8` gives writePPM's bytes (tone-mapped on each device before the gather)."""
        f64 = params.precision == capi.PRECISION_F64
        out = np.empty((params.height, params.width, 3), dtype=np.uint8 if u8 else (np.float64 if f64 else np.float32))
        st = capi.RenderStats()
        fn = (self._lib.rayz_hip_multi_render_u8 if u8 else
              self._lib.rayz_hip_multi_render_f64 if f64 else self._lib.rayz_hip_multi_render)
        rc = fn(self._h, C.byref(camera), C.byref(params), out.ctypes.data_as(C.c_void_p), C.byref(st))
        capi.check(self._lib, rc, "rayz_hip_multi_render")
        return out, st

    def device_stats(self):
        """Per-device counters of the last frame (each device's own trace-kernel time: shard imbalance shows here)."""
        out = []
        for i in range(len(self.devices)):
            st = capi.RenderStats()
            capi.check(self._lib, self._lib.rayz_hip_multi_device_stats(self._h, i, C.byref(st)), "rayz_hip_multi_device_stats")
            out.append(st)
        return out

    def timing(self):
        """(gather_ms, frame_ms) of the last frame: see include/rayz_hip.h."""
        g, f = C.c_double(), C.c_double()
        capi.check(self._lib, self._lib.rayz_hip_multi_timing(self._h, C.byref(g), C.byref(f)), "rayz_hip_multi_timing")
        return g.value, f.value


def kat(op: int, records, precision: int = capi.PRECISION_F32) -> np.ndarray:
    """`rayz_hip_kat`: the trace kernels' own device functions on (n, KAT_IN_STRIDE) float64 records."""
    lib = capi.load()
    rec = np.ascontiguousarray(records, dtype=np.float64).reshape(-1, capi.KAT_IN_STRIDE)
    out = np.zeros((len(rec), capi.KAT_OUT_STRIDE))
    D = C.POINTER(C.c_double)
    capi.check(lib, lib.rayz_hip_kat(op, precision, rec.ctypes.data_as(D), len(rec), out.ctypes.data_as(D)), "rayz_hip_kat")
    return out


def noise_kat(chunk_sums, chunk_sizes, precision: int = capi.PRECISION_F32, rel_error: float | None = None,
              mean_floor: float | None = None):
    """`rayz_hip_noise_kat`: the noise kernels on (n_chunks, n_pixels, 3) float64 chunk sums with `chunk_sizes` samples each.
    Returns (Q (n_pixels, 3), var, rel2 (n_pixels,) float64, capi.NoiseSummary)."""
    lib = capi.load()
    sums = np.ascontiguousarray(chunk_sums, dtype=np.float64)
    if sums.ndim != 3 or sums.shape[2] != 3:
        raise ValueError(f"chunk_sums must be (n_chunks, n_pixels, 3), got {sums.shape}")
    sizes = np.ascontiguousarray(chunk_sizes, dtype=np.uint32)
    if sizes.shape != (sums.shape[0],):
        raise ValueError(f"chunk_sizes must be ({sums.shape[0]},), got {sizes.shape}")
    k, n = sums.shape[:2]
    q, var, rel2 = np.zeros((n, 3)), np.zeros(n), np.zeros(n)
    prm, sm = Progressive._noise_params(rel_error, mean_floor), capi.NoiseSummary()
    D = C.POINTER(C.c_double)
    rc = lib.rayz_hip_noise_kat(precision, sums.ctypes.data_as(D), sizes.ctypes.data_as(C.POINTER(C.c_uint32)), n, k, C.byref(prm),
                                q.ctypes.data_as(D), var.ctypes.data_as(D), rel2.ctypes.data_as(D), C.byref(sm))
    capi.check(lib, rc, "rayz_hip_noise_kat")
    return q, var, rel2, sm


def adaptive_kat(chunk_sums, chunk_sizes, pass_ends, precision: int = capi.PRECISION_F32, rel_error: float | None = None,
                 mean_floor: float | None = None, min_chunks: int = capi.ADAPTIVE_DEFAULT_MIN_CHUNKS, width: int = 0):
    """`rayz_hip_adaptive_kat`: fold, freeze and compaction of adaptive passes on (n_chunks, n_pixels, 3) float64 chunk sums; pass p
    ends at chunk count pass_ends[p].  Returns a dict: frozen_at (n_pixels,) uint32; acc, Q, frame (n_pixels, 3) float64; lists — the
    active list every pass traced, then what is left (len(pass_ends) + 1 uint32 arrays)."""
    lib = capi.load()
    sums = np.ascontiguousarray(chunk_sums, dtype=np.float64)
    if sums.ndim != 3 or sums.shape[2] != 3:
        raise ValueError(f"chunk_sums must be (n_chunks, n_pixels, 3), got {sums.shape}")
    sizes = np.ascontiguousarray(chunk_sizes, dtype=np.uint32)
    if sizes.shape != (sums.shape[0],):
        raise ValueError(f"chunk_sizes must be ({sums.shape[0]},), got {sizes.shape}")
    ends = np.ascontiguousarray(pass_ends, dtype=np.uint32)
    k, n = sums.shape[:2]
    frozen = np.zeros(n, dtype=np.uint32)
    acc, q, frame = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros((n, 3))
    lists, lens = np.zeros((len(ends) + 1, max(n, 1)), dtype=np.uint32), np.zeros(len(ends) + 1, dtype=np.uint32)
    prm = Progressive._noise_params(rel_error, mean_floor)
    D, U = C.POINTER(C.c_double), C.POINTER(C.c_uint32)
    rc = lib.rayz_hip_adaptive_kat(precision, sums.ctypes.data_as(D), sizes.ctypes.data_as(U), n, k, ends.ctypes.data_as(U), len(ends), width,
                                   min_chunks, C.byref(prm), frozen.ctypes.data_as(U), acc.ctypes.data_as(D), q.ctypes.data_as(D),
                                   frame.ctypes.data_as(D), lists.ctypes.data_as(U) if n else None, lens.ctypes.data_as(U))
    capi.check(lib, rc, "rayz_hip_adaptive_kat")
    return {"frozen_at": frozen, "acc": acc, "Q": q, "frame": frame, "lists": [lists[p, :lens[p]].copy() for p in range(len(ends) + 1)]}


def tonemap_u8(rgb_ptr: int, out_ptr: int, n_pixels: int, stream: int = 0) -> None:
    lib = capi.load()
    capi.check(lib, lib.rayz_hip_tonemap_u8(C.c_void_p(rgb_ptr), C.c_void_p(out_ptr), n_pixels, C.c_void_p(stream)),
               "rayz_hip_tonemap_u8")
