"""The chain G-buffer kernels (rayz_hip_scene_query_camera_chain) on the GPU: every output equals the contract's
restatement (chain_ref.chain) bit for bit, composed from the CPU oracle's pieces AND from the library's own ray queries and
known-answer entry, for the flat list and the BVH in both node formats, f32 and f64, max_depth 0 / 1 / 4 / 16, a tiled frame, an
untiled one and a shard, from outside the glass and from inside it."""
import numpy as np
import pytest
import torch

import chain_ref
import chain_scenes as cs
from rayz_amd import capi

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR, BVH = capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH
FIELDS = ("index", "t", "point", "normal", "front_face", "material", "albedo", "key", "depth", "first_index")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tracers():
    return {c: cs.build(c) for c in cs.CAMERAS}


@pytest.fixture(scope="module")
def references(gpu, oracle, tracers):
    """ref(backend name, camera, precision, max_depth): the chains of the whole 64x40 frame, each computed once (the backends keep
    every ray's record, so the shorter chains cost nothing after the longest)."""
    backends, scenes, done = {}, {}, {}

    def ref(which, cam, precision, max_depth):
        key = (which, cam, precision, max_depth)
        if key not in done:
            t = tracers[cam]
            if (which, cam, precision) not in backends:
                if which == "oracle":
                    be = chain_ref.OracleBackend(oracle, t.scene_desc(), precision)
                else:
                    scenes[cam] = scenes.get(cam) or gpu.DeviceScene(t.scene_desc())
                    be = chain_ref.DeviceBackend(gpu, scenes[cam], t.scene_desc(), precision, LINEAR)
                backends[(which, cam, precision)] = be
                px, py = cs.shape_pixels(cs.W, cs.H)
                chain_ref.chain(be, t.camera_desc(), px, py, cs.TMIN, max(cs.DEPTHS), cs.MAX_FUZZ)  # (the longest first)
            px, py = cs.shape_pixels(cs.W, cs.H)
            done[key] = chain_ref.chain(backends[(which, cam, precision)], t.camera_desc(), px, py, cs.TMIN, max_depth, cs.MAX_FUZZ)
        return done[key]

    yield ref
    for s in scenes.values():
        s.close()


def bits_of(a, precision, field):
    """An output as integers: floats by their bit patterns (so -0 differs from +0)."""
    a = np.asarray(a)
    if field in ("t", "point", "normal", "albedo"):
        return np.ascontiguousarray(a, np.float32).view(np.uint32) if precision == F32 else np.ascontiguousarray(a, np.float64).view(np.uint64)
    if field == "key":
        return a.astype(np.int64) & 0xFFFFFFFF
    return a.astype(np.int64)


def got_of(g, field):
    return getattr(g, field).cpu().numpy().reshape((-1, 3) if field in ("point", "normal", "albedo") else (-1,))


@pytest.mark.parametrize("precision", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("traversal,node_format", [(LINEAR, 0), (BVH, 1), (BVH, 2)], ids=["flat", "bvh-planes", "bvh-indices"])
def test_chain_kernels_equal_the_contract(gpu, references, tracers, traversal, node_format, precision):
    gpu.debug_set(capi.DEBUG_BVH_NODES, node_format)
    try:
        for cam in cs.CAMERAS:
            t = tracers[cam]
            scene = gpu.DeviceScene(t.scene_desc())  # (a fresh scene: the node format acts when the tree is built)
            try:
                for max_depth in cs.DEPTHS:
                    refs = {w: references(w, cam, precision, max_depth) for w in ("oracle", "device")}
                    for shape, (w, h, shard) in cs.SHAPES.items():
                        p = cs.frame_params(t, precision, traversal, w, h, shard)
                        g = scene.gbuffer(t.camera_desc(), p, chain=dict(max_depth=max_depth, max_fuzz=cs.MAX_FUZZ))
                        st = scene.query_sync()
                        assert g.is_chain
                        px, py = cs.shape_pixels(w, h, shard)
                        at = py * cs.W + px
                        what = f"{cam} camera, max_depth {max_depth}, {shape}"
                        for which, r in refs.items():
                            for f in FIELDS:
                                got, want = bits_of(got_of(g, f), precision, f), bits_of(r[f][at], precision, f)
                                bad = np.nonzero((got != want).reshape(len(at), -1).any(axis=1))[0]
                                assert not len(bad), (f"{what}: {f} differs from the {which} composition at {len(bad)} pixels, first "
                                                      f"(px, py) = {(int(px[bad[0]]), int(py[bad[0]]))}: got {got_of(g, f)[bad[0]]}, "
                                                      f"want {r[f][at][bad[0]]}")
                        assert st.primary_rays == len(at) and st.segments == int(refs["oracle"]["segments"][at].sum()), what
            finally:
                scene.close()
    finally:
        gpu.debug_set(capi.DEBUG_BVH_NODES, 0)


def test_the_frames_show_every_case(references):
    """Not skipped: at least 16 pixels of each case in the 64x40 frames of the two cameras together, at every max_depth that can show
    it (test_chain_cpu.py checks the same without a GPU)."""
    for precision in (F32, F64):
        for max_depth in cs.DEPTHS:
            n = {}
            for cam in cs.CAMERAS:
                for k, v in cs.classes(references("oracle", cam, precision, max_depth), max_depth).items():
                    n[k] = n.get(k, 0) + v
            need = ["at max_depth on a specular record", "stopped by max_fuzz"] + (["a miss after a followed hit", "total internal reflection"]
                                                                                   if max_depth >= 1 else []) + (["depth >= 2"] if max_depth >= 2 else [])
            for k in need:
                assert n[k] >= 16, (precision, max_depth, k, n)


@pytest.mark.parametrize("precision", [F32, F64], ids=["f32", "f64"])
@pytest.mark.parametrize("traversal", [LINEAR, BVH], ids=["flat", "bvh"])
def test_max_depth_0_is_the_camera_query(gpu, tracers, traversal, precision):
    for cam in cs.CAMERAS:
        t = tracers[cam]
        scene = gpu.DeviceScene(t.scene_desc())
        try:
            for shape, (w, h, shard) in cs.SHAPES.items():
                p = cs.frame_params(t, precision, traversal, w, h, shard)
                a = scene.gbuffer(t.camera_desc(), p)
                sa = scene.query_sync()
                b = scene.gbuffer(t.camera_desc(), p, chain=dict(max_depth=0))
                sb = scene.query_sync()
                for f in gpu.QUERY_OUTPUTS:
                    x, y = getattr(a, f), getattr(b, f)
                    same = torch.equal(x.view(torch.int32 if x.dtype == torch.float32 else torch.int64), y.view(torch.int32 if y.dtype == torch.float32 else torch.int64)) \
                        if x.is_floating_point() else torch.equal(x, y)
                    assert same, (cam, shape, f)
                assert not b.key.any() and not b.depth.any() and torch.equal(b.first_index, a.index), (cam, shape)
                assert (sb.primary_rays, sb.segments) == (sa.primary_rays, sa.segments) == (a.index.numel(), a.index.numel())
                assert (sb.node_tests, sb.sphere_tests) == (sa.node_tests, sa.sphere_tests)
        finally:
            scene.close()


@pytest.mark.parametrize("traversal", [LINEAR, BVH], ids=["flat", "bvh"])
def test_a_chain_call_between_two_renders_changes_no_frame(gpu, tracers, traversal):
    t = tracers["outside"]
    scene = gpu.DeviceScene(t.scene_desc())
    try:
        p = cs.frame_params(t, F32, traversal)
        p.samples_per_px, p.max_bounces, p.seed = 4, 8, 5
        dev = torch.device("cuda", scene.device)
        frames = [torch.zeros((cs.H, cs.W, 3), dtype=torch.float32, device=dev) for _ in range(2)]
        torch.cuda.synchronize(dev)
        scene.render_into(t.camera_desc(), p, frames[0].data_ptr())
        st0 = scene.sync()
        g = scene.gbuffer(t.camera_desc(), p, chain=True)
        q = scene.query_sync()
        assert q.segments > q.primary_rays == cs.W * cs.H and int(g.depth.max()) == capi.CHAIN_DEFAULTS["max_depth"]
        st_mid = scene.sync()  # (the render's counters, not the chain's)
        assert (st_mid.primary_rays, st_mid.segments) == (st0.primary_rays, st0.segments)
        scene.render_into(t.camera_desc(), p, frames[1].data_ptr())
        st1 = scene.sync()
        assert torch.equal(frames[0].view(torch.int32), frames[1].view(torch.int32)) and frames[0].abs().sum() > 0
        assert (st1.primary_rays, st1.segments) == (st0.primary_rays, st0.segments)
    finally:
        scene.close()


def test_python_layer_of_chain_results(gpu, tracers):
    """gbuffer(chain=...) validates its parameters, marks its result, and the temporal handle refuses it."""
    t = tracers["outside"]
    scene = gpu.DeviceScene(t.scene_desc())
    try:
        p = cs.frame_params(t, F32, LINEAR)
        with pytest.raises(ValueError, match="chain"):
            scene.gbuffer(t.camera_desc(), p, chain=dict(depth=3))
        with pytest.raises(ValueError, match="chain"):
            scene.gbuffer(t.camera_desc(), p, chain=3)
        with pytest.raises(capi.RayzHipError, match="max_depth"):
            scene.gbuffer(t.camera_desc(), p, chain=dict(max_depth=17))
        g = scene.gbuffer(t.camera_desc(), p, chain=True)
        scene.query_sync()
        first = scene.gbuffer(t.camera_desc(), p)
        scene.query_sync()
        assert g.is_chain and not first.is_chain and first.key is None
        assert g.key.dtype == torch.int32 and g.depth.dtype == torch.uint8 and g.first_index.dtype == torch.int32
        assert tuple(g.key.shape) == tuple(g.depth.shape) == tuple(g.first_index.shape) == (cs.H, cs.W)
        rgb = torch.zeros((cs.H, cs.W, 3), dtype=torch.float32, device=g.key.device)
        tm = gpu.Temporal(cs.W, cs.H)
        try:
            with pytest.raises(ValueError, match="first-hit"):
                tm.step(rgb, rgb, g, t.camera_desc(), 4)
            tm.step(rgb, rgb, first, t.camera_desc(), 4)
        finally:
            tm.close()
        mm = gpu.Temporal(cs.W, cs.H, moments=True)
        try:
            with pytest.raises(ValueError, match="first-hit"):
                mm.step_moments(rgb, g, t.camera_desc(), 4)
        finally:
            mm.close()
    finally:
        scene.close()
