"""Primary lists on the device: primary_lists_kernel builds each pixel's candidate list, the primary_*_kernels
resolve every path's camera segment from it.  One DeviceScene per scene; per precision and forced scan form (XZ, XY, ONE_RADIUS)
the frame with the lists OFF and ON, each held byte for byte to oracle mode B, the segments too (so to each other).  48x27 frames at
8 spp, the scenes of tests/primary_lists_scenes.py and the launch shapes the list phase can go wrong at: a frame that is all sky
(every chunk ends inside list phases), one bounce, lanes with and without lists in one wave (overflow), an interleaved shard, fewer
items than a wave grabs, a moved camera, a progressive handle in four passes; AUTO's two gates through the getter."""
import numpy as np
import pytest

import primary_lists_scenes as S
from helpers import assert_images_equal
from rayz_amd import capi, dist, render, tracer
from test_reuse_gpu import Want, camera, out_tensor, params

pytestmark = pytest.mark.gpu

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR = capi.TRAVERSAL_LINEAR
FORMS = (capi.SCAN_FORM_XZ, capi.SCAN_FORM_XY, capi.SCAN_FORM_ONE_RADIUS)
AUTO, OFF, ON = capi.PRIMARY_LISTS_AUTO, capi.PRIMARY_LISTS_OFF, capi.PRIMARY_LISTS_ON
MIN_SPHERES, MIN_SPP = 1024, 128  # plane_runs.hpp: kPrimaryMinSpheres, kPrimaryMinSpp


def render_once(ds, cam, p):
    out = out_tensor(p)
    ds.render_into(cam, p, out.data_ptr())
    st = ds.sync()
    return out.cpu().numpy(), st.segments


def check(gpu, oracle, t, what, cams=None, rows=None, precisions=(F32, F64), forms=FORMS, **kw):
    """OFF and ON under every form == the oracle's frame (its `rows`, for a shard) and segments, for each camera in turn."""
    scene = t.scene_desc()
    want = Want(oracle, scene)
    ds = gpu.DeviceScene(scene)
    try:
        for prec in precisions:
            for form in forms:
                ds.scan_form = form
                for mode in (OFF, ON):
                    ds.set_primary_lists(mode)
                    for k, cam in enumerate(cams or [t.camera_desc()]):
                        p = params(t.params(), traversal=LINEAR, precision=prec, **kw)
                        assert ds.uses_primary_lists(p.samples_per_px) == (mode == ON)
                        got, seg = render_once(ds, cam, p)
                        tag = f"{what}: precision {prec}, form {form}, lists {mode}, camera {k}"
                        if rows is None:
                            ref, ost = want(cam, p)
                            assert_images_equal(got, ref, tag)
                            assert seg == ost.segments, (tag, seg, ost.segments)
                        else:  # a shard: the oracle's frame is the whole one; the segments are held OFF against ON
                            ref, _ = want(cam, params(p, shard_index=0, shard_count=1, tile_rows=0))
                            assert_images_equal(got, ref[rows], tag)
                            if mode == OFF:
                                seg_off = seg
                            assert seg == seg_off, (tag, seg, seg_off)
    finally:
        ds.close()


@pytest.mark.parametrize("name", S.NAMES)
def test_lists_off_and_on_render_the_oracles_frame_under_every_form(gpu, oracle, name):
    check(gpu, oracle, S.build(name), name)


def test_a_frame_that_is_all_sky_ends_with_the_queue_drained(gpu, oracle):
    """Every pixel's list is empty (tests/test_primary_lists_cpu.py holds that): no lane ever reaches a scan."""
    check(gpu, oracle, S.build("all_sky"), "all sky")


def test_one_bounce(gpu, oracle):
    check(gpu, oracle, S.build("defocus_mixed"), "max_bounces 1", max_bounces=1)


@pytest.mark.parametrize("rank", [0, 2])
def test_an_interleaved_shard(gpu, oracle, rank):
    t = S.build("pinhole_mixed")
    p = dist.shard_params(t.params(), rank, 3)
    rows = render.shard_row_indices(S.H, 8, rank, 3)
    assert 0 < len(rows) < S.H and render.shard_rows(p) == len(rows)
    check(gpu, oracle, t, f"rank {rank} of 3", rows=rows, tile_rows=p.tile_rows, shard_index=rank, shard_count=3)


def test_fewer_items_than_one_wave_grabs(gpu, oracle):
    t = S.build("pinhole_mixed")
    cam = camera(oracle, ((3.0, 5.0, 13.0), 40.0, 10.0), 8, 4)  # 32 pixels, one chunk each: 32 items, a wave grabs 64
    check(gpu, oracle, t, "8x4", cams=[cam], width=8, height=4)


def test_the_lists_follow_a_moved_camera(gpu, oracle):
    t = S.build("defocus_mixed")
    a = t.camera_desc()
    b = camera(oracle, ((-9.0, 3.0, 9.0), 35.0, 12.0), S.W, S.H)
    check(gpu, oracle, t, "moved camera", cams=[a, b, a])


@pytest.mark.parametrize("prec", [F32, F64])
def test_a_progressive_handle_in_four_passes_ends_in_the_one_shot_frame(gpu, oracle, prec):
    t = S.build("overflow", spp=32)
    scene, cam = t.scene_desc(), t.camera_desc()
    p = params(t.params(), traversal=LINEAR, precision=prec, chunk_spp=8)
    ds = gpu.DeviceScene(scene)
    try:
        ds.set_primary_lists(ON)
        one_shot, seg = render_once(ds, cam, p)
        ref, ost = oracle.render_b(scene, cam, p)
        assert_images_equal(one_shot, ref, "one shot")
        assert seg == ost.segments
        pr = ds.progressive(cam, p)
        try:
            assert pr.n_chunks == 4
            passes = 0
            while not pr.done:
                out = out_tensor(p)
                pr.step(0, out.data_ptr())  # one chunk per pass; the lists are built by the first
                passes += 1
                if passes == 2:  # another camera's one-shot render in between leaves the handle's lists alone
                    render_once(ds, camera(oracle, ((-9.0, 3.0, 9.0), 35.0, 12.0), S.W, S.H), p)
            st = pr.stats()
            assert passes == 4
            assert_images_equal(out.cpu().numpy(), one_shot, "four passes")
            assert st.segments == seg
        finally:
            pr.close()
    finally:
        ds.close()


def _pool(n):
    t = tracer.Tracer.init(S.W, 40.0, 10.0, 0.0, (0.0, 4.0, 14.0), (0.0, 0.0, 0.0), (0, 1, 0), seed=3)
    m = t.pool.add_diffuse(t.pool.add_solid_texture((0.5, 0.5, 0.5)), 0)
    rng = np.random.default_rng(n)
    for _ in range(n):
        t.pool.add_sphere(tuple(rng.uniform(-8, 8, 3)), 0.1, int(m))
    return t


def test_autos_two_gates(gpu):
    for n, spp, on in [(MIN_SPHERES, MIN_SPP, True), (MIN_SPHERES - 1, MIN_SPP, False), (MIN_SPHERES, MIN_SPP - 1, False),
                       (MIN_SPHERES - 1, 1 << 20, False), (4 * MIN_SPHERES, 1, False)]:
        t = _pool(n)
        ds = gpu.DeviceScene(t.scene_desc())
        try:
            assert ds.uses_primary_lists(spp) == on, (n, spp)
            ds.set_primary_lists(ON)
            assert ds.uses_primary_lists(1)
            ds.set_primary_lists(OFF)
            assert not ds.uses_primary_lists(1 << 20)
            ds.set_primary_lists(AUTO)
            assert ds.uses_primary_lists(spp) == on
            with pytest.raises(capi.RayzHipError):
                ds.set_primary_lists(3)
        finally:
            ds.close()
