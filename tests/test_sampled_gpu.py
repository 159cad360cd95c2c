"""The sampled G-buffer kernels (rayz_hip_scene_query_camera_sampled) on the GPU: every output equals the
contract's restatement (sampled_ref) bit for bit, composed from the CPU oracle's pieces AND from the library's own ray queries and
known-answer entry, for the flat list and the BVH in both node formats, f32 and f64, n = 1 / 2 / 5 of 5 samples per pixel, a tiled
frame, an untiled one and a shard, through a lens and a pinhole; n = 1 is a ray query of the same rays; a render of one bounce is
black exactly where every sample hits; a call between two renders changes neither; and the Python layer."""
import itertools

import numpy as np
import pytest
import torch

import sampled_ref
import sampled_scenes as ss
from rayz_amd import capi

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR, BVH = capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH
FIELDS = ("albedo", "normal", "t", "hits")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tracers():
    return {c: ss.build(c) for c in ss.CAMERAS}


@pytest.fixture(scope="module")
def references(gpu, oracle, tracers):
    """ref(backend name, camera, precision, width, height): every sample's record of the whole frame of that width (path ids depend
    on the width), each computed once."""
    scenes, done = {}, {}

    def ref(which, cam, precision, width, height):
        key = (which, cam, precision, width, height)
        if key not in done:
            t = tracers[cam]
            if which == "oracle":
                be = sampled_ref.OracleBackend(oracle, t.scene_desc(), precision)
            else:
                scenes[cam] = scenes.get(cam) or gpu.DeviceScene(t.scene_desc())
                be = sampled_ref.DeviceBackend(gpu, scenes[cam], t.scene_desc(), precision, LINEAR)
            px, py = ss.shape_pixels(width, height)
            done[key] = sampled_ref.records(be, oracle, t.camera_desc(), px, py, width, ss.SPP, ss.SEED, ss.TMIN)
        return done[key]

    yield ref
    for s in scenes.values():
        s.close()


def bits_of(a, precision, field):
    """An output as integers: floats by their bit patterns (so -0 differs from +0)."""
    a = np.asarray(a)
    if field == "hits":
        return a.astype(np.int64)
    return np.ascontiguousarray(a, np.float32).view(np.uint32) if precision == F32 else np.ascontiguousarray(a, np.float64).view(np.uint64)


def got_of(g, field):
    return getattr(g, field).cpu().numpy().reshape((-1, 3) if field in ("albedo", "normal") else (-1,))


@pytest.mark.parametrize("precision", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("traversal,node_format", [(LINEAR, 0), (BVH, 1), (BVH, 2)], ids=["flat", "bvh-planes", "bvh-indices"])
def test_sampled_kernels_equal_the_contract(gpu, references, tracers, traversal, node_format, precision):
    gpu.debug_set(capi.DEBUG_BVH_NODES, node_format)
    try:
        for cam in ss.CAMERAS:
            t = tracers[cam]
            scene = gpu.DeviceScene(t.scene_desc())  # (a fresh scene: the node format acts when the tree is built)
            try:
                for shape, (w, h, shard) in ss.SHAPES.items():
                    recs = {which: references(which, cam, precision, w, h) for which in ("oracle", "device")}
                    px, py = ss.shape_pixels(w, h, shard)
                    at = py * w + px
                    p = ss.frame_params(t, precision, traversal, w, h, shard)
                    for n in ss.SAMPLES:
                        g = scene.gbuffer_sampled(t.camera_desc(), p, samples=n)
                        st = scene.query_sync()
                        what = f"{cam} camera, n {n}, {shape}"
                        assert g.samples == n
                        for which, rec in recs.items():
                            want = sampled_ref.means({k: v[at] for k, v in rec.items()}, n, precision)
                            for f in FIELDS:
                                a, b = bits_of(got_of(g, f), precision, f), bits_of(want[f], precision, f)
                                bad = np.nonzero((a != b).reshape(len(at), -1).any(axis=1))[0]
                                assert not len(bad), (f"{what}: {f} differs from the {which} composition at {len(bad)} pixels, first "
                                                      f"(px, py) = {(int(px[bad[0]]), int(py[bad[0]]))}: got {got_of(g, f)[bad[0]]}, "
                                                      f"want {want[f][bad[0]]}")
                        assert st.primary_rays == st.segments == len(at) * n, what
                        assert (st.node_tests > 0) == (traversal == BVH) and st.sphere_tests > 0, what
            finally:
                scene.close()
    finally:
        gpu.debug_set(capi.DEBUG_BVH_NODES, 0)


def test_the_frames_show_every_case(references):
    """Not skipped (test_sampled_cpu.py checks the same without a GPU): the frames the kernels were held to show every case."""
    for precision in (F32, F64):
        for w, h, _ in ss.SHAPES.values():
            for cam in ss.CAMERAS:
                n = ss.classes(references("oracle", cam, precision, w, h), ss.SPP)
                for k, v in n.items():
                    assert v > 0 or (k == "samples with more than one lens try" and cam == "pinhole"), (precision, w, h, cam, n)


@pytest.mark.parametrize("precision", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("traversal", [LINEAR, BVH], ids=["flat", "bvh"])
def test_one_sample_is_the_query_of_its_ray(gpu, references, tracers, traversal, precision):
    """n = 1 against DeviceScene.query of the reference's rays: 0 + x and x / 1 are x but for the sign of a zero, and a miss's
    albedo is 1 where a query writes 0."""
    dt = torch.float32 if precision == F32 else torch.float64
    for cam in ss.CAMERAS:
        t = tracers[cam]
        scene = gpu.DeviceScene(t.scene_desc())
        try:
            for shape, (w, h, shard) in ss.SHAPES.items():
                px, py = ss.shape_pixels(w, h, shard)
                rays = references("oracle", cam, precision, w, h)["rays"][py * w + px, 0]
                q = scene.query(torch.tensor(rays, dtype=dt, device=torch.device("cuda", scene.device)), tmin=ss.TMIN, traversal=traversal,
                                outputs=("index", "t", "normal", "albedo"))
                scene.query_sync()
                g = scene.gbuffer_sampled(t.camera_desc(), ss.frame_params(t, precision, traversal, w, h, shard), samples=1)
                scene.query_sync()
                hit = q.index >= 0
                zero = torch.zeros((), dtype=dt, device=hit.device)
                assert torch.equal(g.hits.reshape(-1), hit.to(torch.int32)), (cam, shape)
                view = torch.int32 if precision == F32 else torch.int64
                for f, want in (("t", q.t), ("normal", q.normal + zero), ("albedo", torch.where(hit[:, None], q.albedo + zero, 1 + zero))):
                    assert torch.equal(getattr(g, f).reshape(want.shape).view(view), want.contiguous().view(view)), (cam, shape, f)
        finally:
            scene.close()


@pytest.mark.parametrize("traversal", [LINEAR, BVH], ids=["flat", "bvh"])
@pytest.mark.parametrize("n", [1, 3])
def test_a_one_bounce_render_is_black_where_every_sample_hits(gpu, tracers, traversal, n):
    """The path ids are the render's: render_into with max_bounces = 1 and samples_per_px = n gives (0, 0, 0) exactly where
    hits = n (a path that hits ends at the bounce limit; a miss adds the sky) — test_sampled_cpu.py shows the premise on the oracle."""
    t = tracers["lens"]
    scene = gpu.DeviceScene(t.scene_desc())
    try:
        for precision, dt in ((F32, torch.float32), (F64, torch.float64)):
            p = ss.frame_params(t, precision, traversal, spp=n)
            dev = torch.device("cuda", scene.device)
            frame = torch.full((ss.H, ss.W, 3), -1.0, dtype=dt, device=dev)
            torch.cuda.synchronize(dev)
            scene.render_into(t.camera_desc(), p, frame.data_ptr())
            scene.sync()
            g = scene.gbuffer_sampled(t.camera_desc(), p, outputs=("hits",))
            scene.query_sync()
            black = (frame == 0).all(dim=2)
            assert torch.equal(black, g.hits == n) and bool((frame[~black] > 0).all())
            assert 0 < int(black.sum()) < black.numel() and (n == 1 or int(((g.hits > 0) & (g.hits < n)).sum()) > 0)
    finally:
        scene.close()


@pytest.mark.parametrize("traversal", [LINEAR, BVH], ids=["flat", "bvh"])
def test_a_sampled_call_between_two_renders_changes_no_frame(gpu, tracers, traversal):
    t = tracers["lens"]
    scene = gpu.DeviceScene(t.scene_desc())
    try:
        p = ss.frame_params(t, F32, traversal)
        p.samples_per_px, p.max_bounces, p.seed = 4, 8, 5
        dev = torch.device("cuda", scene.device)
        frames = [torch.zeros((ss.H, ss.W, 3), dtype=torch.float32, device=dev) for _ in range(2)]
        torch.cuda.synchronize(dev)
        scene.render_into(t.camera_desc(), p, frames[0].data_ptr())
        st0 = scene.sync()
        g = scene.gbuffer_sampled(t.camera_desc(), p)
        q = scene.query_sync()
        assert q.segments == q.primary_rays == ss.W * ss.H * 4 and int(g.hits.max()) == 4 and int(g.hits.min()) == 0
        st_mid = scene.sync()  # (the render's counters, not the sampled call's)
        assert (st_mid.primary_rays, st_mid.segments) == (st0.primary_rays, st0.segments)
        scene.render_into(t.camera_desc(), p, frames[1].data_ptr())
        st1 = scene.sync()
        assert torch.equal(frames[0].view(torch.int32), frames[1].view(torch.int32)) and frames[0].abs().sum() > 0
        assert (st1.primary_rays, st1.segments) == (st0.primary_rays, st0.segments)
    finally:
        scene.close()


def test_python_layer_of_sampled_results(gpu, tracers):
    """Shapes, dtypes, every subset of the outputs (`normal` alone needs the count it does not return), the refusals, and
    with_albedo in front of a filter."""
    t = tracers["lens"]
    scene = gpu.DeviceScene(t.scene_desc())
    try:
        for precision, dt in ((F32, torch.float32), (F64, torch.float64)):
            p = ss.frame_params(t, precision, LINEAR, 50, 37, (1, 3))
            rows = gpu.shard_rows(p)
            full = scene.gbuffer_sampled(t.camera_desc(), p)
            scene.query_sync()
            assert full.samples == ss.SPP
            assert tuple(full.albedo.shape) == tuple(full.normal.shape) == (rows, 50, 3) and tuple(full.t.shape) == tuple(full.hits.shape) == (rows, 50)
            assert full.albedo.dtype == full.normal.dtype == full.t.dtype == dt and full.hits.dtype == torch.int32
            view = torch.int32 if precision == F32 else torch.int64
            for k in range(len(FIELDS) + 1):
                for subset in itertools.combinations(FIELDS, k):
                    for traversal in (LINEAR, BVH):
                        p.traversal = traversal
                        g = scene.gbuffer_sampled(t.camera_desc(), p, outputs=subset)
                        scene.query_sync()
                        for f in FIELDS:
                            if f not in subset:
                                assert getattr(g, f) is None, (subset, f)
                            elif f == "hits":
                                assert torch.equal(g.hits, full.hits), subset
                            else:
                                assert torch.equal(getattr(g, f).view(view), getattr(full, f).view(view)), (subset, f)
        p = ss.frame_params(t, F32, LINEAR)
        with pytest.raises(ValueError, match="sampled output"):
            scene.gbuffer_sampled(t.camera_desc(), p, outputs=("albedo", "index"))
        for bad in (0, -1, 2.0, True):
            with pytest.raises(ValueError, match="samples"):
                scene.gbuffer_sampled(t.camera_desc(), p, samples=bad)
        with pytest.raises(capi.RayzHipError, match="samples 6 > samples_per_px 5"):
            scene.gbuffer_sampled(t.camera_desc(), p, samples=ss.SPP + 1)
        p.samples_per_px = 0
        with pytest.raises(capi.RayzHipError, match="samples_per_px"):
            scene.gbuffer_sampled(t.camera_desc(), p)
        # with_albedo: the one line in front of a filter's DENOISE_ALBEDO
        p = ss.frame_params(t, F32, LINEAR)
        first = scene.gbuffer(t.camera_desc(), p)
        scene.query_sync()
        s = scene.gbuffer_sampled(t.camera_desc(), p, outputs=("albedo",))
        scene.query_sync()
        guide = first.with_albedo(s.albedo)
        assert guide.albedo is s.albedo and guide.index is first.index and first.albedo is not s.albedo
        rgb = torch.rand((ss.H, ss.W, 3), dtype=torch.float32, device=s.albedo.device)
        dn = gpu.Denoiser(ss.W, ss.H)
        try:
            a = dn.run(rgb, guide, flags=capi.DENOISE_ALBEDO)
            b = dn.run(rgb, first, flags=capi.DENOISE_ALBEDO)
            torch.cuda.synchronize()
            assert tuple(a.shape) == tuple(rgb.shape) and bool(torch.isfinite(a).all()) and not torch.equal(a, b)
        finally:
            dn.close()
        with pytest.raises(ValueError, match="with_albedo"):
            first.with_albedo(s.albedo.to(torch.float64))
    finally:
        scene.close()
