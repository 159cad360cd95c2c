"""Handles that live across frames, against the oracle: one `DeviceScene` and one `MultiScene` driven through scripted
sequences of changing renders, and the host mirror's cached multi-device handle.

Almost every other parity test renders through the one-shot entry (fresh scene, one render, destroyed).  bench.py, the Zig
drop-in and `Tracer.render()` with a device list keep their handles, and a reused handle carries state from one render to
the next: the grow-only chunk-sum workspace, the device copy of the chunk schedule, the filter padding of each buffer set
(rebuilt when a camera needs a larger origin bound), the BVH buffers, the stream of the previous render and the counters
`sync()` reports; a multi handle adds grow-only tiles, `gathered` and `frame` buffers.  Every render here is compared bit
for bit with oracle mode B for that render's own arguments, so a stale piece of that state shows as wrong pixels or
counters.  No step frees or shrinks a buffer an earlier, unsynchronised render may still use: renders that run without a
host sync in between share one frame size and one chunk schedule."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from helpers import assert_images_equal, check_counters
from rayz_amd import capi, render, tracer

pytestmark = pytest.mark.gpu

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR, BVH, AUTO = capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH, capi.TRAVERSAL_AUTO
NEAR = ((0.0, 4.0, 18.0), 40.0, 18.0)  # look_from, vfov, focus distance (looking at the origin)
# 20,000 units out with a 0.065 degree field: the pool fills the frame and the origin bound rises ~1,000x.  A camera a few
# thousand units out leaves only 0-4 pixels of this frame to the filter padding of the near camera; at 20,000 a render on
# buffers padded for the near camera loses grazing hits in ~15-25 pixels (the oracle's own filter at both bounds; on the
# device: 15 pixels of the f32 flat-list frame).
FAR = (tuple(20000.0 * x for x in np.array([0.55, 0.3, 0.78]) / np.linalg.norm([0.55, 0.3, 0.78])), 0.065, 20000.0)


def pool_tracer(seed=5):
    """400 spheres (static / y-moving / generally moving) and 8 triangles in a 18 x 10 x 18 box around the origin, every
    material kind: more than RAYZ_AUTO_BVH_MIN hittables and no ground sphere, so the origin bound is about 15 and the near
    camera's (|look_from| ~ 18.4) sets the first filter padding."""
    rng = np.random.default_rng(seed)
    (lf, vfov, focus) = NEAR
    t = tracer.Tracer.init(96, vfov, focus, 0.0, lf, (0, 0, 0), (0, 1, 0), seed=seed)
    P = t.pool
    tex = [P.add_solid_texture(rng.uniform(0.1, 0.9, 3)) for _ in range(4)]
    tex.append(P.add_checker_texture(0.7, tex[0], tex[1]))
    mats = [P.add_diffuse(tex[k], k % 3) for k in range(5)]
    mats += [P.add_metallic(tex[2], 0.0), P.add_metallic(tex[3], 0.4), P.add_dielectric(1.5)]
    for k in range(400):
        c = rng.uniform((-9, -5, -9), (9, 5, 9))
        v = ((0, 0, 0) if k % 3 == 0 else (0, float(rng.uniform(-1, 1)), 0) if k % 3 == 1
             else tuple(rng.uniform(-0.6, 0.6, 3)))
        P.add_sphere(c, float(rng.uniform(0.2, 0.6)), int(mats[k % len(mats)]), velocity=v)
    for _ in range(8):
        a = rng.uniform((-8, -4, -8), (8, 4, 8))
        P.add_triangle(a, a + rng.uniform(-2, 2, 3), a + rng.uniform(-2, 2, 3), int(rng.choice(mats)))
    t.samples_per_px, t.max_bounces = 4, 8
    t.set_gpu(render_seed=11)
    return t


def camera(oracle, view, w, h):
    lf, vfov, focus = view
    c = capi.CameraDesc()
    oracle.load().rayz_oracle_camera_init(vfov, focus, 0.0, capi.D3(*lf), capi.D3(0, 0, 0), capi.D3(0, 1, 0), h, w, c)
    return c


def params(base, **kw):
    p = capi.RenderParams.from_buffer_copy(bytes(base))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def schedule(p):
    buf = (C.c_uint32 * 64)()
    n = capi.load().rayz_hip_chunk_schedule(C.byref(p), buf, 64)
    return list(buf[: n + 1])


class Want:
    """Oracle mode B for one pool, memoised on (camera, params)."""

    def __init__(self, oracle, scene):
        self.oracle, self.scene, self.memo = oracle, scene, {}

    def __call__(self, cam, p):
        key = bytes(cam) + bytes(p)
        if key not in self.memo:
            self.memo[key] = self.oracle.render_b(self.scene, cam, p)
        return self.memo[key]


def check_stats(st, ost, p, what):
    rows = render.shard_rows(p)
    assert st.primary_rays == ost.primary_rays == rows * p.width * p.samples_per_px, (what, st.primary_rays, ost.primary_rays)
    assert st.segments == ost.segments, (what, st.segments, ost.segments)
    check_counters(st, ost)


def out_tensor(p):
    """The render's output, pre-filled with NaN (every value must be written); made on torch's stream, so synchronised
    before a library stream that does not wait for torch's."""
    dt = torch.float64 if p.precision == F64 else torch.float32
    out = torch.full((render.shard_rows(p), p.width, 3), float("nan"), dtype=dt, device="cuda")
    torch.cuda.synchronize()
    return out


def render_checked(ds, want, cam, p, what, stream=0):
    out = out_tensor(p)
    ds.render_into(cam, p, out.data_ptr(), stream)
    st = ds.sync()
    got = out.cpu().numpy()
    ref, ost = want(cam, p)
    assert_images_equal(got, ref, what)
    check_stats(st, ost, p, what)
    return got, st


# ---- 1. one DeviceScene through a scripted sequence ------------------------------------------------------------------------
def test_device_scene_through_a_changing_sequence(gpu, oracle):
    t = pool_tracer()
    scene = t.scene_desc()
    assert scene.n_spheres + scene.n_triangles > 160 and scene.n_triangles > 0
    want = Want(oracle, scene)
    near, far = camera(oracle, NEAR, 96, 54), camera(oracle, FAR, 160, 90)
    base = params(t.params(), width=96, height=54)
    ds = gpu.DeviceScene(scene)
    try:
        # 1-2. the first upload (scan streams), then the first BVH build on it, then AUTO (picks the BVH here)
        p = params(base, traversal=LINEAR)
        first, _ = render_checked(ds, want, near, p, "step 1: f32 linear")
        _, st = render_checked(ds, want, near, params(p, traversal=BVH), "step 2: f32 BVH")
        assert st.node_tests > 0
        _, st = render_checked(ds, want, near, params(p, traversal=AUTO), "step 2: f32 AUTO")
        assert st.node_tests > 0
        # 3. the f64 buffer set (sharing the narrow-phase buffers), BVH first this time
        render_checked(ds, want, near, params(p, precision=F64, traversal=BVH), "step 3: f64 BVH")
        render_checked(ds, want, near, params(p, precision=F64, traversal=LINEAR), "step 3: f64 linear")
        # 4. more chunk sums per pixel on a larger frame: the workspace and the chunk table grow; f64 grows the workspace again
        big_cam = camera(oracle, NEAR, 160, 90)
        pb = params(base, width=160, height=90, samples_per_px=8, chunk_spp=1, traversal=AUTO)
        assert len(schedule(pb)) == 9
        render_checked(ds, want, big_cam, pb, "step 4: 160x90, 8 chunks per pixel, f32")
        render_checked(ds, want, big_cam, params(pb, precision=F64), "step 4: 160x90, 8 chunks per pixel, f64")
        # 5. chunk tables of the same length and different contents, back to back
        small_cam = camera(oracle, NEAR, 48, 27)
        p17 = params(base, width=48, height=27, samples_per_px=17, chunk_spp=16)
        p20 = params(p17, samples_per_px=20)
        assert schedule(p17) == [0, 16, 17] and schedule(p20) == [0, 16, 20]
        for k, q in enumerate((p17, p20, p17)):
            render_checked(ds, want, small_cam, q, f"step 5.{k}: chunk table {schedule(q)}")
        # 6. row shards (one of them without rows), then the whole frame again
        pw = params(base, traversal=AUTO)
        whole, _ = render_checked(ds, want, near, pw, "step 6: whole frame")
        for tile, count, idxs in ((1, 3, (0, 2, 1)), (5, 12, (3, 11, 0))):  # 54 rows in 5-row tiles: 11 tiles, shard 11 has none
            for idx in idxs:
                q = params(pw, tile_rows=tile, shard_index=idx, shard_count=count)
                got, st = render_checked(ds, want, near, q, f"step 6: shard {idx} of {count}, {tile}-row tiles")
                assert_images_equal(got, whole[render.shard_row_indices(54, tile, idx, count)], "step 6: shard rows")
                if render.shard_rows(q) == 0:
                    assert (tile, count, idx) == (5, 12, 11) and st.primary_rays == 0 and st.segments == 0
        render_checked(ds, want, near, pw, "step 6: whole frame after the shards")
        # 7. max_bounces = 0 (an early return): black, and sync() reports this render, not the previous one
        q = params(pw, max_bounces=0, samples_per_px=3)
        got, st = render_checked(ds, want, near, q, "step 7: max_bounces 0")
        assert (got == 0).all()
        _, hst = gpu.render_host(scene, near, q)
        assert (st.primary_rays, st.segments, st.sphere_tests, st.node_tests) == \
               (hst.primary_rays, hst.segments, hst.sphere_tests, hst.node_tests) == (96 * 54 * 3, 0, 0, 0)
        render_checked(ds, want, near, pw, "step 7: whole frame after max_bounces 0")
        # 8. a distant camera raises the origin bound: both buffer sets re-padded, the BVH rebuilt; then the near camera on
        #    the over-padded buffers
        pf = params(base, width=160, height=90, samples_per_px=8)
        for prec in (F32, F64):
            for trav in (LINEAR, BVH):
                render_checked(ds, want, far, params(pf, precision=prec, traversal=trav),
                               f"step 8: distant camera, precision {prec}, traversal {trav}")
        for prec in (F32, F64):
            for trav in (LINEAR, BVH):
                render_checked(ds, want, near, params(p, precision=prec, traversal=trav),
                               f"step 8: near camera again, precision {prec}, traversal {trav}")
        assert_images_equal(render_checked(ds, want, near, p, "step 8: step 1 again")[0], first, "step 8: step 1 again")
        # 9. three streams without a host sync in between (same frame and schedule: nothing is reallocated meanwhile)
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        pa, pb2, pc = (params(pw, seed=s) for s in (101, 202, 303))
        outs = [out_tensor(q) for q in (pa, pb2, pc)]
        ds.render_into(near, pa, outs[0].data_ptr(), s1.cuda_stream)
        ds.render_into(near, pb2, outs[1].data_ptr(), s2.cuda_stream)
        ds.render_into(near, pc, outs[2].data_ptr(), 0)
        st = ds.sync()
        torch.cuda.synchronize()
        for q, o, name in zip((pa, pb2, pc), outs, ("A on s1", "B on s2", "C on the library stream")):
            assert_images_equal(o.cpu().numpy(), want(near, q)[0], f"step 9: {name}")
        check_stats(st, want(near, pc)[1], pc, "step 9: counters of C")
        # 10. process-wide scheduling knobs changed between renders on the live scene: the same images
        try:
            for knob, value in ((capi.DEBUG_QUEUE_GRAB, 256), (capi.DEBUG_BVH_KEEP, 1 | (1 << 8)), (capi.DEBUG_LDS_PAD, 40 * 1024),
                                (capi.DEBUG_QUEUE_GRAB, 32), (capi.DEBUG_BVH_KEEP, 64 | (64 << 8)), (capi.DEBUG_LDS_PAD, 8 * 1024)):
                render.debug_set(knob, value)
                for prec in (F32, F64):
                    render_checked(ds, want, near, params(pw, precision=prec, traversal=BVH), f"step 10: knob {knob} = {value}")
        finally:
            for knob in (capi.DEBUG_QUEUE_GRAB, capi.DEBUG_BVH_KEEP, capi.DEBUG_LDS_PAD):
                render.debug_set(knob, -1)
        render_checked(ds, want, near, params(pw, traversal=BVH), "step 10: knobs back to their defaults")
    finally:
        ds.close()


def test_device_scene_copies_the_pool_at_create(gpu, oracle):
    """11. The handle holds its own copy: a sphere added to the Tracer's pool after create does not reach it."""
    t, t0 = pool_tracer(), pool_tracer()  # t0: the same generator and seed, never mutated (the oracle's pool)
    near = camera(oracle, NEAR, 96, 54)
    p = params(t.params(), width=96, height=54)
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        m = t.pool.add_diffuse(t.pool.add_solid_texture((0.9, 0.1, 0.1)))
        t.pool.add_sphere((0, 0, 0), 3.0, m)
        assert t.info().n_spheres == t0.info().n_spheres + 1
        mutated, _ = oracle.render_b(t.scene_desc(), near, p)
        want = Want(oracle, t0.scene_desc())
        got, _ = render_checked(ds, want, near, p, "pool copied at create")
        assert not np.array_equal(got, mutated)  # (the added sphere is in view)
    finally:
        ds.close()


def test_two_device_scenes_alive_at_once(gpu, oracle):
    """Two handles interleaved on one stream and on separate streams, with different frame shapes and schedules: each
    keeps its own workspace, chunk table and counters."""
    ta, tb = pool_tracer(), tracer.randomBouncing(64, -4, 4, seed=9)
    tb.samples_per_px, tb.max_bounces = 5, 9
    tb.set_gpu(render_seed=4)
    sa, sb = ta.scene_desc(), tb.scene_desc()
    wa, wb = Want(oracle, sa), Want(oracle, sb)
    ca, cb = camera(oracle, NEAR, 96, 54), tb.camera_desc()
    pa = params(ta.params(), width=96, height=54, samples_per_px=6, chunk_spp=2, traversal=BVH)
    pb = params(tb.params(), traversal=LINEAR, precision=F64)
    da, db = gpu.DeviceScene(sa), gpu.DeviceScene(sb)
    shared, s1, s2 = torch.cuda.Stream(), torch.cuda.Stream(), torch.cuda.Stream()
    try:
        for rnd, (xa, xb) in enumerate(((shared, shared), (s1, s2), (s2, s1), (shared, shared))):
            qa, qb = params(pa, seed=10 + rnd), params(pb, seed=20 + rnd)
            oa, ob = out_tensor(qa), out_tensor(qb)
            da.render_into(ca, qa, oa.data_ptr(), xa.cuda_stream)
            db.render_into(cb, qb, ob.data_ptr(), xb.cuda_stream)
            stb, sta = db.sync(), da.sync()
            torch.cuda.synchronize()
            assert_images_equal(oa.cpu().numpy(), wa(ca, qa)[0], f"round {rnd}: scene A")
            assert_images_equal(ob.cpu().numpy(), wb(cb, qb)[0], f"round {rnd}: scene B")
            check_stats(sta, wa(ca, qa)[1], qa, f"round {rnd}: scene A counters")
            check_stats(stb, wb(cb, qb)[1], qb, f"round {rnd}: scene B counters")
            assert sta.node_tests > 0 and stb.node_tests == 0
    finally:
        da.close()
        db.close()


# ---- 2. one MultiScene through a sequence ----------------------------------------------------------------------------------
@pytest.mark.parametrize("devices,transport", [([0], capi.GATHER_RCCL),
                                               ([0] * 8, capi.GATHER_PEER_COPY | capi.GATHER_ALLOW_DUPLICATE_DEVICES)],
                         ids=["n1-rccl", "n8-peer"])
def test_multi_scene_through_a_changing_sequence(gpu, oracle, devices, transport):
    t = pool_tracer()
    scene = t.scene_desc()
    want = Want(oracle, scene)
    base = params(t.params(), traversal=AUTO)
    n = len(devices)
    m = render.MultiScene(scene, devices, transport)

    def frame(w, h, what, u8=False, **kw):
        cam = camera(oracle, NEAR, w, h)
        p = params(base, width=w, height=h, **kw)
        got, st = m.render(cam, p, u8=u8)
        ref, ost = want(cam, p)
        if u8:
            img = tracer.Image(h, w)
            img.pixels = ref.astype(np.float64)
            ref = img.to_u8()
        assert_images_equal(got, ref, what)
        check_stats(st, ost, p, what)
        per = m.device_stats()
        assert len(per) == n
        for f in ("primary_rays", "segments", "sphere_tests", "node_tests"):
            assert sum(getattr(d, f) for d in per) == getattr(st, f), (what, f)
        tile = p.tile_rows or 8
        for i, d in enumerate(per):  # every shard's own rows (none: nothing launched, nothing counted)
            rows = len(render.shard_row_indices(h, tile, i, n))
            assert d.primary_rays == rows * w * p.samples_per_px, (what, i)
            assert rows > 0 or d.segments == 0
        gather_ms, frame_ms = m.timing()
        assert math.isfinite(gather_ms) and math.isfinite(frame_ms) and gather_ms >= 0 and frame_ms >= 0, (gather_ms, frame_ms)
        return got, per

    try:
        first, _ = frame(96, 54, "96x54 f32")
        frame(160, 90, "160x90 f32: tiles, gathered and frame grow")
        frame(64, 36, "64x36 f64, 1-row tiles", precision=F64, tile_rows=1)
        assert (39 * 70 * 3) % 256 and (8 * 70 * 3) % 256  # neither the whole frame nor an 8-row tile is 256-byte aligned
        frame(70, 39, "70x39 u8", u8=True)
        _, per = frame(32, 9, "32x9 f32 in 8-row tiles: shards without rows", tile_rows=8)
        if n == 8:
            assert [d.primary_rays == 0 for d in per] == [False, False] + [True] * 6
        got, _ = frame(96, 54, "max_bounces 0", max_bounces=0, samples_per_px=3)
        assert (got == 0).all()
        again, _ = frame(96, 54, "96x54 f32 again")
        assert_images_equal(again, first, "the first frame again")
    finally:
        m.close()


# ---- 3. the host mirror's cached multi-device handle -----------------------------------------------------------------------
def test_tracer_render_keeps_its_multi_handle_right(gpu, oracle):
    """`Tracer.render()` with a device list caches one RayzMulti (rebuilt when the pool or the list changes); every frame
    equals the oracle of the pool as it is at that render."""
    t = pool_tracer()
    t.set_gpu(devices=[0])

    def frame(what):
        p = t.params()
        rays = t.render()
        want, ost = oracle.render_b(t.scene_desc(), t.camera_desc(), p)
        assert rays == p.width * p.height * p.samples_per_px
        assert_images_equal(t.img.pixels.astype(np.float32), want, what)
        assert (t.img.pixels == want.astype(np.float64)).all()
        assert t.stats.segments == ost.segments
        return want

    before = frame("devices [0]: first render")
    m = t.pool.add_metallic(t.pool.add_solid_texture((0.9, 0.9, 0.2)), 0.0)
    t.pool.add_sphere((0, 0, 0), 3.0, m)
    after = frame("devices [0]: after adding a sphere")
    assert not np.array_equal(before, after)  # (the new sphere is in view: a stale cached handle would show)
    frame("devices [0]: unchanged")
    t.set_gpu(devices=[])
    frame("single device")
    t.set_gpu(devices=[0])
    frame("devices [0] again")
