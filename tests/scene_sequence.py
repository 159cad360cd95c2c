"""One live scene driven through scripted sequences of query-side and render-side calls (test_scene_sequences_gpu.py runs them,
test_scene_sequences_cpu.py checks on the CPU that they show what they claim): a raw call layer over the C ABI, and the expected
answers.

`DeviceScene`'s Python methods wait for the previous query before every new one (`_query_prologue`), so through them no two
query-side calls are ever in flight behind each other.  The C API allows exactly that (include/rayz_hip.h: calls on one stream
queue, a call on another stream first waits for the scene's last launch), and the host code has paths that exist for that case
alone.  The callers here go to `capi.load()` on the scene's handle and wait for nothing.

  Call         what to issue: kind, camera, params, precision, traversal, extra arguments, stream
  alloc        a call's output tensors (every field of its kind, prefilled, requested or not) and its input tensors
  issue        the library call itself; raises capi.RayzHipError on a refusal
  expected     the same call on a FRESH scene, followed at once by its sync: outputs on the host and counters, memoised
  check        a call's buffers against `expected`, bit pattern for bit pattern; a field not requested still holds its prefill

A fresh scene carries no history, and every kind is held to the oracle or to an exact restatement on a fresh scene by its own test
(test_query_exact_gpu, test_chain_gpu, test_sampled_gpu, test_sparse_gpu, test_reuse_gpu); a full render's fresh frame is also
compared with oracle mode B here."""
import ctypes as C
from dataclasses import dataclass

import numpy as np

import query_reference as qr
import sampled_ref
import sampled_scenes as ss
from rayz_amd import capi, render

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR, BVH = capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH
ALL = 0xFFFFFFFF
SENTINEL, HITS_PREFILL = -7, 0x7FFFFFFF  # what an integer field and `hits` hold before a call (floats: NaN)
W, H = ss.W, ss.H
SHAPES = ss.SHAPES  # "64x40 tiled", "50x37 untiled" (lanes past the frame, tiled_pixels < n), "64x40 shard 1 of 3"
# 20,000 units out, level with the scene: rays above y = 0 pass over the ground sphere (sky, or one of the small hittables), rays
# below hit it.  The field of view spans about 9.6 x 6 units at the scene.  (test_reuse_gpu.FAR's distance, aimed at this scene.)
FAR_FROM, FAR_AT, FAR_VFOV = (12000.0, 1.0, 16000.0), (0.0, 1.0, 0.0), 0.0172
FAR_RAYS_OUT = 3000.0

# field -> (element type, vector length): "R" is the call's precision
QUERY_FIELDS = {"index": ("i32", 1), "t": ("R", 1), "point": ("R", 3), "normal": ("R", 3), "front_face": ("u8", 1), "material": ("i32", 1),
                "albedo": ("R", 3), "hit": ("u8", 1)}
CHAIN_FIELDS = {**QUERY_FIELDS, "key": ("i32", 1), "depth": ("u8", 1), "first_index": ("i32", 1)}
SAMPLED_FIELDS = {"albedo": ("R", 3), "normal": ("R", 3), "t": ("R", 1), "hits": ("i32", 1)}
FIELDS = {"query": QUERY_FIELDS, "camera": QUERY_FIELDS, "chain": CHAIN_FIELDS, "sampled": SAMPLED_FIELDS, "render": {"rgb": ("R", 3)},
          "sparse": {"rgb": ("R", 3), "var": ("f32", 3)}}
DEFAULT_OUTPUTS = {"query": render.QUERY_OUTPUTS, "camera": render.QUERY_OUTPUTS, "chain": render.QUERY_OUTPUTS + render.CHAIN_OUTPUTS,
                   "sampled": render.SAMPLED_OUTPUTS, "render": ("rgb",)}
QUERY_KINDS = ("query", "camera", "chain", "sampled")  # rayz_hip_query_sync waits for these, rayz_hip_scene_sync for the others
COUNTERS = ("primary_rays", "segments", "sphere_tests", "node_tests")


@dataclass(frozen=True)
class Call:
    kind: str               # "query", "camera", "chain", "sampled", "render" or "sparse"
    cam: str = "lens"       # a key of Context.cameras ("lens", "pinhole", "far"); a batch query has no camera
    params: tuple = ()      # RenderParams fields as (name, value) pairs, over sampled_scenes.frame_params
    precision: int = F32
    traversal: int = LINEAR
    extra: tuple = ()       # (name, value) pairs: samples | max_depth, max_fuzz | outputs | rays, query | pixels, dest, var
    stream: int = 0         # a hipStream_t as int; 0: the library's stream

    def key(self):
        """What the answer depends on (not the stream)."""
        return (self.kind, self.cam, self.params, self.precision, self.traversal, self.extra)

    def arg(self, name, default=None):
        return dict(self.extra).get(name, default)

    @property
    def outputs(self):
        if self.kind == "sparse":
            return ("rgb", "var") if self.arg("var") else ("rgb",)
        if self.kind == "query" and self.arg("query", "nearest") == "any":
            return ("hit",)
        return tuple(self.arg("outputs", DEFAULT_OUTPUTS[self.kind]))

    def on(self, stream):
        return Call(self.kind, self.cam, self.params, self.precision, self.traversal, self.extra, int(stream))

    def __str__(self):
        extra = ", ".join(f"{k}={v}" for k, v in self.extra)
        return (f"{self.kind}({self.cam}, {dict(self.params)}, {'f64' if self.precision == F64 else 'f32'}, "
                f"{'BVH' if self.traversal == BVH else 'flat'}{', ' + extra if extra else ''})")


def call(kind, cam="lens", shape="64x40 tiled", precision=F32, traversal=LINEAR, params=None, **extra):
    w, h, (si, sc) = SHAPES[shape]
    p = {"width": w, "height": h, "shard_index": si, "shard_count": sc, **(params or {})}
    if kind == "query":
        cam, p = "", {}
    return Call(kind, cam, tuple(sorted(p.items())), precision, traversal, tuple(sorted(extra.items())))


# ---- the scripts (lists of calls; the GPU tests run them, the CPU test inspects them) ---------------------------------------------
RENDER = {"samples_per_px": 4, "max_bounces": 8}  # test 3's frames
SPARSE_OTHER = {"samples_per_px": 20, "chunk_spp": 3, "max_bounces": 8}  # .. and the sparse render between its handle's steps
HANDLE = {"samples_per_px": 6, "chunk_spp": 1, "max_bounces": 8}  # six chunks


def one_stream():
    """Test 1: nine query-side calls queued on the library's stream."""
    return [call("camera"),
            call("chain", traversal=BVH, max_depth=4, max_fuzz=0.25),
            call("sampled", shape="50x37 untiled", samples=5),
            call("sampled", precision=F64, traversal=BVH, samples=2),
            call("query", traversal=BVH, rays="r1000", query="nearest"),
            call("sampled", cam="pinhole", samples=1),
            call("chain", max_depth=2, max_fuzz=0.25, outputs=("index", "albedo", "normal", "key", "depth")),
            call("query", precision=F64, rays="r257", query="any"),
            call("sampled", shape="64x40 shard 1 of 3", samples=5, outputs=("hits", "t"))]


def three_streams():
    """Test 2: six calls rotating kind and stream (the indices 1, 2, 0: s1, s2, the library's)."""
    return [(call("chain", max_depth=4, max_fuzz=0.25), 1), (call("sampled", traversal=BVH, samples=5), 2), (call("camera", cam="pinhole"), 0),
            (call("sampled", precision=F64, samples=3), 1), (call("chain", traversal=BVH, max_depth=3, max_fuzz=0.0, outputs=("t", "point", "first_index")), 2),
            (call("query", rays="r1000", query="nearest", outputs=("index", "t", "albedo")), 0)]


def same_kind_back_to_back():
    """Two chain calls, then two sampled calls, each pair with different outputs and nothing between them: the stores record is
    rewritten behind a kernel of the same kind that is still reading it."""
    return [call("chain", traversal=BVH, max_depth=4, max_fuzz=0.25),
            call("chain", cam="pinhole", max_depth=1, max_fuzz=0.25, outputs=("t", "material", "depth")),
            call("sampled", samples=5),
            call("sampled", cam="pinhole", shape="50x37 untiled", traversal=BVH, samples=3, outputs=("albedo", "hits"))]


def among_renders(precision):
    """Test 3, first part: render, sampled, sparse, chain, render."""
    return [call("render", precision=precision, params={**RENDER, "seed": 7}),
            call("sampled", precision=precision, params={**RENDER, "seed": 7}, samples=4),
            call("sparse", precision=precision, params={**RENDER, "seed": 7}, pixels="s300", dest=True, var=precision == F32),
            call("chain", precision=precision, traversal=BVH, max_depth=4, max_fuzz=0.25),
            call("render", precision=precision, params={**RENDER, "seed": 8})]


def between_steps(precision):
    """Test 3, second part: what is issued while a progressive handle is half way."""
    other = F32 if precision == F64 else F64
    return [call("sampled", precision=other, samples=5),
            call("sparse", precision=precision, params=SPARSE_OTHER, pixels="s300", dest=True, var=precision == F32),
            call("chain", cam="pinhole", precision=precision, max_depth=4, max_fuzz=0.25)]


def handle_params(precision):
    return call("render", precision=precision, traversal=BVH, params=HANDLE)


def near_calls(traversals):
    """All three G-buffer kinds in both precisions; traversals[k % len] for the k-th."""
    calls = []
    for precision in (F32, F64):
        for kind, extra in (("camera", {}), ("chain", {"max_depth": 4, "max_fuzz": 0.25}), ("sampled", {"samples": 5})):
            calls.append(call(kind, precision=precision, traversal=traversals[len(calls) % len(traversals)], **extra))
    return calls


def growing_bound():
    """Test 4: (near calls, the far batch, the far camera's calls, the near calls again on both traversals)."""
    far_batch = [call("query", traversal=BVH, rays="far", query="nearest")]
    far_cam = [call("sampled", cam="far", traversal=BVH, samples=5), call("chain", cam="far", precision=F64, traversal=BVH, max_depth=4, max_fuzz=0.25),
               call("sampled", cam="far", precision=F64, samples=2), call("chain", cam="far", max_depth=4, max_fuzz=0.25)]
    return near_calls((LINEAR, BVH)), far_batch, far_cam, near_calls((LINEAR,)) + near_calls((BVH,))


def first_calls():
    """Test 5: one of each kind; each is some scene's very first call."""
    return [call("query", rays="r257", query="nearest"), call("camera", traversal=BVH), call("chain", max_depth=4, max_fuzz=0.25),
            call("sampled", traversal=BVH, samples=5)]


def refusals():
    """Test 5: (the call in flight, the three refused calls with the text of their refusal, the next accepted call of each kind)."""
    in_flight = call("sampled", traversal=BVH, samples=5)
    refused = [(call("sampled", samples=ss.SPP + 1), "samples 6 > samples_per_px 5"),
               (call("query", rays="nan1000", query="nearest"), "NaN or infinite origin"),
               (call("sparse", params=RENDER, pixels="out of range", dest=False, var=True), "outside the shard")]
    accepted = [call("query", rays="r1000", query="any"), call("camera"), call("chain", traversal=BVH, max_depth=4, max_fuzz=0.25),
                call("sampled", samples=2), call("sparse", params=RENDER, pixels="s300", dest=False, var=True)]
    return in_flight, refused, accepted


def every_call():
    """Every accepted call of every script (the CPU test walks these)."""
    calls = one_stream() + [c for c, _ in three_streams()] + same_kind_back_to_back() + first_calls()
    for precision in (F32, F64):
        calls += among_renders(precision) + between_steps(precision) + [handle_params(precision)]
    for part in growing_bound():
        calls += part
    in_flight, _, accepted = refusals()
    return calls + [in_flight] + accepted


# ---- the scene, its cameras, rays and pixel lists ------------------------------------------------------------------------------------
class Context:
    """sampled_scenes' pool with its two cameras and the far one, and the named ray batches and pixel lists."""

    def __init__(self, oracle):
        self.oracle = oracle
        self.tracers = {c: ss.build(c) for c in ss.CAMERAS}  # (kept alive: the scene description points into the pool)
        self.scene = self.tracers["lens"].scene_desc()
        self.cameras = {c: t.camera_desc() for c, t in self.tracers.items()}
        far = capi.CameraDesc()
        oracle.load().rayz_oracle_camera_init(FAR_VFOV, float(np.linalg.norm(np.subtract(FAR_FROM, FAR_AT))), 0.0, capi.D3(*FAR_FROM),
                                              capi.D3(*FAR_AT), capi.D3(0, 1, 0), H, W, far)
        self.cameras["far"] = far
        self._rays, self._lists = {}, {}

    def params(self, c: Call) -> capi.RenderParams:
        p = ss.frame_params(self.tracers["lens"], c.precision, c.traversal)
        for k, v in c.params:
            setattr(p, k, v)
        return p

    def _sample_rays(self, cam, precision, count, seed):
        """The reference's per-sample rays of `count` pixels of the 64x40 frame (their sample 0: jittered over pixel, lens, shutter)."""
        at = np.random.default_rng(seed).permutation(W * H)[:count]
        be = sampled_ref.OracleBackend(self.oracle, self.scene, precision)
        rec = sampled_ref.records(be, self.oracle, self.cameras[cam], at % W, at // W, W, ss.SPP, ss.SEED, ss.TMIN, n=1)
        return rec["rays"][:, 0]

    @staticmethod
    def _misses(count, origin):
        """Rays that leave upwards from above every hittable."""
        k = np.arange(count)
        rays = np.zeros((count, 8))
        rays[:, 0:3], rays[:, 3], rays[:, 7] = origin, (k % 4) / 4.0, np.inf
        rays[:, 4], rays[:, 5], rays[:, 6] = np.cos(k), 1.0 + k / 8.0, np.sin(k)
        return rays

    def rays(self, name, precision):
        """(n, 8) float64 holding values of the precision: {ox, oy, oz, time, dx, dy, dz, tmax}."""
        key = (name, precision)
        if key not in self._rays:
            if name == "r1000":  # 1,000 rays
                r = np.concatenate([self._sample_rays("lens", precision, 988, 21), self._misses(12, (0.0, 6.0, 0.0))])
            elif name == "r257":  # one past a workgroup
                r = np.concatenate([self._sample_rays("pinhole", precision, 250, 22), self._misses(7, (1.0, 5.0, -2.0))])
            elif name == "nan1000":  # refused after its bound kernel ran: one NaN origin in the last ray
                r = self.rays("r1000", precision).copy()
                r[-1, 0] = np.nan
            elif name == "far":  # origins 3,000 units out, aimed at points in and around the scene, and a few that leave upwards
                rng = np.random.default_rng(23)
                o = FAR_RAYS_OUT * np.array([0.6, 0.0, 0.8]) + np.c_[rng.uniform(-1, 1, 56), rng.uniform(0.5, 1.5, 56), rng.uniform(-1, 1, 56)]
                target = np.c_[rng.uniform(-3, 2.5, 56), rng.uniform(-0.5, 2.5, 56), rng.uniform(0, 5, 56)]
                r = np.zeros((56, 8))
                r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, rng.uniform(0, 1, 56), target - o, np.inf
                r = np.concatenate([r, self._misses(8, tuple(FAR_RAYS_OUT * np.array([0.6, 0.002, 0.8])))])
            else:
                raise KeyError(name)
            self._rays[key] = qr.narrow(r, precision)
        return self._rays[key]

    def pixels(self, name):
        """(pixel list, dest or None when the call scatters nowhere, the output's slot count with dest)."""
        if name not in self._lists:
            rng = np.random.default_rng(24)
            if name == "s300":  # 300 pixels of the 64x40 frame with duplicates, scattered over a frame of 64x40 slots
                px = rng.integers(0, W * H, 300)
                px[1], px[299] = px[0], px[150]
                self._lists[name] = (px.astype(np.int32), rng.permutation(W * H)[:300].astype(np.int32), W * H)
            elif name == "out of range":  # one entry equal to the shard's pixel count
                px = rng.integers(0, W * H, 50)
                px[17] = W * H
                self._lists[name] = (px.astype(np.int32), None, 50)
            else:
                raise KeyError(name)
        return self._lists[name]


_context = None


def context(oracle) -> Context:
    global _context
    if _context is None:
        _context = Context(oracle)
    return _context


# ---- buffers ---------------------------------------------------------------------------------------------------------------------------
class Buffers:
    """A call's tensors: `out` (field -> tensor, every field of the kind) and `inputs` (rays; pixels, dest), owned by the test."""

    def __init__(self, c: Call):
        self.call, self.out, self.inputs = c, {}, {}


def _prefilled(shape, elem, name, precision):
    import torch

    if elem == "R":
        return torch.full(shape, float("nan"), dtype=torch.float64 if precision == F64 else torch.float32, device="cuda")
    if elem == "f32":
        return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    if elem == "u8":
        return torch.full(shape, SENTINEL & 0xFF, dtype=torch.uint8, device="cuda")
    return torch.full(shape, HITS_PREFILL if name == "hits" else SENTINEL, dtype=torch.int32, device="cuda")


def alloc(ctx: Context, c: Call) -> Buffers:
    """Made on torch's stream: call torch.cuda.synchronize() once after all allocations and before the first library call (the
    library's stream does not wait for torch's, test_reuse_gpu.out_tensor)."""
    import torch

    b = Buffers(c)
    if c.kind == "query":
        rays = ctx.rays(c.arg("rays"), c.precision)
        b.inputs["rays"] = torch.tensor(rays, dtype=torch.float64 if c.precision == F64 else torch.float32, device="cuda")
        shape = (len(rays),)
    elif c.kind == "sparse":
        px, dest, slots = ctx.pixels(c.arg("pixels"))
        b.inputs["pixels"] = torch.tensor(px, dtype=torch.int32, device="cuda")
        if c.arg("dest"):
            b.inputs["dest"] = torch.tensor(dest, dtype=torch.int32, device="cuda")
        shape = (slots if c.arg("dest") else len(px),)
    else:
        p = ctx.params(c)
        shape = (render.shard_rows(p), p.width)
    for name, (elem, vec) in FIELDS[c.kind].items():
        b.out[name] = _prefilled(shape + ((3,) if vec == 3 else ()), elem, name, c.precision)
    return b


def _pointers(struct, b: Buffers, names):
    o = struct()
    for k in names:
        if k in b.call.outputs:
            setattr(o, k, b.out[k].data_ptr())
    return o


def issue(ds, ctx: Context, c: Call, b: Buffers) -> None:
    """The library call of `c` on the handle of `ds`, writing `b`; nothing is waited for."""
    lib = capi.load()
    h, stream = ds._h, C.c_void_p(c.stream or None)
    if c.kind == "query":
        n = int(b.inputs["rays"].shape[0])
        q = capi.QueryParams(n_rays=n, kind=capi.QUERY_ANY if c.arg("query", "nearest") == "any" else capi.QUERY_NEAREST,
                             precision=c.precision, traversal=c.traversal, tmin=ss.TMIN)
        out = _pointers(capi.QueryOutputs, b, QUERY_FIELDS)
        rc = lib.rayz_hip_scene_query(h, C.byref(q), C.c_void_p(b.inputs["rays"].data_ptr()), C.byref(out), stream)
        return capi.check(lib, rc, "rayz_hip_scene_query")
    cam, p = ctx.cameras[c.cam], ctx.params(c)
    if c.kind == "camera":
        out = _pointers(capi.QueryOutputs, b, QUERY_FIELDS)
        rc = lib.rayz_hip_scene_query_camera(h, C.byref(cam), C.byref(p), C.byref(out), stream)
        return capi.check(lib, rc, "rayz_hip_scene_query_camera")
    if c.kind == "chain":
        out, co = _pointers(capi.QueryOutputs, b, QUERY_FIELDS), _pointers(capi.ChainOutputs, b, render.CHAIN_OUTPUTS)
        prm = capi.ChainParams(max_depth=c.arg("max_depth"), max_fuzz=c.arg("max_fuzz"))
        rc = lib.rayz_hip_scene_query_camera_chain(h, C.byref(cam), C.byref(p), C.byref(prm), C.byref(out), C.byref(co), stream)
        return capi.check(lib, rc, "rayz_hip_scene_query_camera_chain")
    if c.kind == "sampled":
        out = _pointers(capi.SampledOutputs, b, SAMPLED_FIELDS)
        prm = capi.SampledParams(samples=c.arg("samples", 0))
        rc = lib.rayz_hip_scene_query_camera_sampled(h, C.byref(cam), C.byref(p), C.byref(prm), C.byref(out), stream)
        return capi.check(lib, rc, "rayz_hip_scene_query_camera_sampled")
    if c.kind == "render":  # (DeviceScene.render_into waits for nothing)
        return ds.render_into(cam, p, b.out["rgb"].data_ptr(), c.stream)
    assert c.kind == "sparse", c.kind
    fn = lib.rayz_hip_scene_render_pixels_f64 if c.precision == F64 else lib.rayz_hip_scene_render_pixels
    dest = b.inputs.get("dest")
    rc = fn(h, C.byref(cam), C.byref(p), C.c_void_p(b.inputs["pixels"].data_ptr()), int(b.inputs["pixels"].numel()),
            C.c_void_p(dest.data_ptr() if dest is not None else None), int(b.out["rgb"].shape[0]), C.c_void_p(b.out["rgb"].data_ptr()),
            C.c_void_p(b.out["var"].data_ptr() if c.arg("var") else None), stream)
    return capi.check(lib, rc, "rayz_hip_scene_render_pixels")


def counters(st: capi.RenderStats) -> dict:
    return {k: int(getattr(st, k)) for k in COUNTERS}


def query_sync(ds) -> dict:
    """rayz_hip_query_sync on the handle (not DeviceScene.query_sync, which also drops the tensors the Python layer keeps)."""
    lib, st = capi.load(), capi.RenderStats()
    capi.check(lib, lib.rayz_hip_query_sync(ds._h, C.byref(st)), "rayz_hip_query_sync")
    return counters(st)


def sync_of(ds, c: Call) -> dict:
    """The sync that reports `c`: the query side's or the render side's."""
    return query_sync(ds) if c.kind in QUERY_KINDS else counters(ds.sync())


# ---- the expected answers ------------------------------------------------------------------------------------------------------------
NODE_FORMAT = 0  # RAYZ_DEBUG_BVH_NODES while a test runs (it acts when a scene's tree is built): part of an answer's key
_memo = {}


def set_node_format(gpu, value: int) -> None:
    global NODE_FORMAT
    gpu.debug_set(capi.DEBUG_BVH_NODES, value)
    NODE_FORMAT = value


def host(b: Buffers) -> dict:
    return {k: t.cpu().numpy() for k, t in b.out.items()}


def expected(gpu, c: Call):
    """(outputs on the host, counters) of `c` as the only call ever made on a fresh scene.  Never modified by a test."""
    import torch

    key = (c.key(), NODE_FORMAT)
    if key not in _memo:
        ctx = _context
        b = alloc(ctx, c)
        torch.cuda.synchronize()
        ds = gpu.DeviceScene(ctx.scene)
        try:
            issue(ds, ctx, c, b)
            st = sync_of(ds, c)
        finally:
            ds.close()
        torch.cuda.synchronize()
        got = host(b)
        if c.kind == "render":  # a fresh scene's frame is the oracle's
            want, ost = ctx.oracle.render_b(ctx.scene, ctx.cameras[c.cam], ctx.params(c))
            bad = int((bits(got["rgb"]) != bits(want)).sum())
            assert bad == 0, f"{c} on a fresh scene: {bad} values differ from oracle mode B"
            assert (st["primary_rays"], st["segments"]) == (ost.primary_rays, ost.segments), (str(c), st, ost.primary_rays, ost.segments)
        for a in got.values():
            a.setflags(write=False)
        _memo[key] = (got, st)
    return _memo[key]


def bits(a):
    """An array as integers: floats by their bit patterns (so -0 differs from +0, and a NaN prefill equals itself)."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype == np.float64:
        return a.view(np.uint64)
    return a


def differences(got: dict, want: dict):
    """[(field, number of differing entries, first differing entry)] of two host copies."""
    out = []
    for k, w in want.items():
        g = got[k]
        assert g.shape == w.shape and g.dtype == w.dtype, (k, g.shape, w.shape, g.dtype, w.dtype)
        vec = 3 if w.ndim >= 2 and w.shape[-1] == 3 else 1  # (no frame here is 3 wide)
        bad = np.nonzero((bits(g) != bits(w)).reshape(-1, vec).any(axis=1))[0]
        if len(bad):
            out.append((k, len(bad), int(bad[0]), g.reshape(-1, vec)[bad[0]].tolist(), w.reshape(-1, vec)[bad[0]].tolist()))
    return out


def check(gpu, b: Buffers, what: str) -> None:
    """Every field of the call's kind equals the fresh scene's, bit for bit — a field not requested: its prefill.  The caller has
    synchronised."""
    want, _ = expected(gpu, b.call)
    bad = differences(host(b), want)
    assert not bad, f"{what}: {b.call} differs from its fresh-scene answer: " + "; ".join(
        f"{k}: {n} entries, first {at}: got {g}, want {w}" for k, n, at, g, w in bad)


def check_prefill(b: Buffers, what: str) -> None:
    """Nothing was written: every field still holds its prefill."""
    for k, t in b.out.items():
        elem, _ = FIELDS[b.call.kind][k]
        want = _prefilled(tuple(t.shape), elem, k, b.call.precision)
        assert not differences({k: t.cpu().numpy()}, {k: want.cpu().numpy()}), f"{what}: {b.call}: {k} was written"
