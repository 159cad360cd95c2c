"""The slab's cells on the device: the cells_*_kernels resolve every listable segment from the outliers and the cells
under the ray's stretch inside the members' slab.  One DeviceScene per scene; per precision, forced scan form (XZ, XY, ONE_RADIUS)
and primary lists OFF / ON the frame with the cells OFF and ON (forced), each held byte for byte to oracle mode B and to the BVH
frame, the segments too (so to each other).  Frames of at most 64x36 at 8 spp, pools of at most 300 spheres, and the shapes the list
phase can go wrong at (the test names say which)."""
import numpy as np
import pytest

from helpers import assert_images_equal
from rayz_amd import capi, dist, render, tracer
from test_reuse_gpu import Want, camera, out_tensor, params

pytestmark = pytest.mark.gpu

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR, BVH = capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH
FORMS = (capi.SCAN_FORM_XZ, capi.SCAN_FORM_XY, capi.SCAN_FORM_ONE_RADIUS)
OFF, ON, AUTO = capi.CELL_LISTS_OFF, capi.CELL_LISTS_ON, capi.CELL_LISTS_AUTO
P_OFF, P_ON = capi.PRIMARY_LISTS_OFF, capi.PRIMARY_LISTS_ON
W, H = 64, 36
MIN_MEMBERS, MAX_OUTLIERS = 1023, 8  # slab_cells.hpp: kCellsMinMembers, kMaxOutliers


def _tracer(seed, look_from, look_at, vfov=40.0):
    t = tracer.Tracer.init(W, vfov, 10.0, 0.0, look_from, look_at, (0, 1, 0), seed=seed)
    P = t.pool
    rng = np.random.default_rng(seed)
    tex = [P.add_solid_texture(rng.uniform(0.1, 0.9, 3)) for _ in range(4)]
    tex.append(P.add_checker_texture(0.5, tex[0], tex[1]))
    mats = [P.add_diffuse(tex[0], 0), P.add_diffuse(tex[4], 1), P.add_diffuse(tex[2], 2), P.add_metallic(tex[3], 0.0),
            P.add_metallic(tex[1], 0.3), P.add_dielectric(1.5)]
    t.samples_per_px, t.max_bounces = 8, 8
    t.set_gpu(render_seed=int(rng.integers(0, 2 ** 62)))
    return t, rng, mats


def _lattice(t, rng, mats, n, r=0.2, half=None):
    """n x n members, one per unit square about the origin, a third of them y-moving."""
    half = n / 2.0 if half is None else half
    for a in range(n):
        for b in range(n):
            vy = float(rng.uniform(0.05, 0.5)) if (a + b) % 3 == 0 else 0.0
            t.pool.add_sphere((a - half + 0.9 * rng.uniform(), r, b - half + 0.9 * rng.uniform()), r, int(mats[(a * n + b) % len(mats)]),
                              velocity=(0.0, vy, 0.0))


def field(look_from=(0.0, 0.45, 12.0), look_at=(0.0, 0.45, 0.0), outliers=2, seed=201):
    """14 x 14 members on a ground; `outliers` hittables that are no members in all (the ground, unit spheres).  Among the members: a
    hollow glass shell, a y-mover that reaches the camera's view only near time 1, and a cell with five centres on the view axis."""
    t, rng, mats = _tracer(seed, look_from, look_at)
    t.pool.add_sphere((0.0, -1000.0, 0.0), 1000.0, int(mats[1]))
    for k in range(outliers - 1):
        t.pool.add_sphere((-7.0 + 2.0 * k, 1.0, -4.0 - (k % 2)), 1.0, int(mats[(3 + k) % len(mats)]))
    _lattice(t, rng, mats, 14)
    t.pool.add_sphere((0.5, 0.3, 5.5), 0.3, int(mats[5]))
    t.pool.add_sphere((0.5, 0.3, 5.5), -0.25, int(mats[5]))  # hollow glass: a negative radius
    t.pool.add_sphere((-1.5, 0.2, 4.5), 0.2, int(mats[0]), velocity=(0.0, 2.5, 0.0))  # in view near time 1 only: the slab reaches 2.9
    for k in range(5):  # an overflowed cell on the camera's path
        t.pool.add_sphere((0.1 + 0.18 * k, 0.1, 8.3 + 0.1 * k), 0.1, int(mats[k % len(mats)]))
    return t


def small_pool_from_above():
    """5 x 5 members the camera looks down on: every stretch inside the slab is short, no segment needs a scan."""
    t, rng, mats = _tracer(202, (0.3, 7.0, 0.2), (0.0, 0.0, 0.0))
    t.pool.add_sphere((0.0, -1000.0, 0.0), 1000.0, int(mats[0]))
    _lattice(t, rng, mats, 5)
    return t


def tall_pool():
    """200 small spheres at heights from -6 to 6 over cells 0.5 wide, seen from the side: a ray's stretch inside that slab runs under
    a dozen cells and more, so hardly a segment is listable."""
    t, rng, mats = _tracer(203, (0.0, 0.5, 14.0), (0.0, 0.0, 0.0))
    for k in range(200):
        t.pool.add_sphere((float(rng.uniform(-4, 4)), float(rng.uniform(-6, 6)), float(rng.uniform(-4, 4))), 0.1, int(mats[k % len(mats)]),
                          velocity=(0.0, float(rng.uniform(0, 0.3)) if k % 4 == 0 else 0.0, 0.0))
    return t


def render_once(ds, cam, p):
    out = out_tensor(p)
    ds.render_into(cam, p, out.data_ptr())
    st = ds.sync()
    return out.cpu().numpy(), st.segments


def check(gpu, oracle, t, what, cams=None, rows=None, precisions=(F32, F64), forms=FORMS, has_cells=True, **kw):
    """Cells OFF and ON under every form, with and without primary lists == the oracle's frame (its `rows`, for a shard), the BVH
    frame and their segments, for each camera in turn."""
    scene = t.scene_desc()
    want = Want(oracle, scene)
    ds = gpu.DeviceScene(scene)
    try:
        for prec in precisions:
            for k, cam in enumerate(cams or [t.camera_desc()]):
                p = params(t.params(), traversal=LINEAR, precision=prec, **kw)
                if rows is None:
                    ref, ost = want(cam, p)
                    ref_seg = ost.segments
                else:  # a shard: the oracle's frame is the whole one; the segments are held to the BVH frame's
                    ref = want(cam, params(p, shard_index=0, shard_count=1, tile_rows=0))[0][rows]
                    ref_seg = None
                bvh, bvh_seg = render_once(ds, cam, params(p, traversal=BVH))
                assert_images_equal(bvh, ref, f"{what}: precision {prec}, camera {k}, BVH")
                ref_seg = bvh_seg if ref_seg is None else ref_seg
                assert bvh_seg == ref_seg
                for form in forms:
                    ds.scan_form = form
                    for pmode in (P_OFF, P_ON):
                        ds.set_primary_lists(pmode)
                        for mode in (OFF, ON):
                            ds.set_cell_lists(mode)
                            assert ds.uses_cell_lists() == (mode == ON and has_cells)
                            got, seg = render_once(ds, cam, p)
                            tag = f"{what}: precision {prec}, form {form}, primary lists {pmode}, cells {mode}, camera {k}"
                            assert_images_equal(got, ref, tag)
                            assert seg == ref_seg, (tag, seg, ref_seg)
    finally:
        ds.close()


def test_a_camera_at_slab_height_looking_along_it(gpu, oracle):
    """Origins inside the slab, the view axis level: d.y changes sign between the two middle rows, whose jittered rays come as
    close to d.y = 0 as f32 lets them (a stretch that does not end: such a ray scans; the exact zero is the CPU test's), stretches
    of every length above and below; the hollow shell, the late y-mover and the overflowed cell in view; rays that leave the grid's
    box on all sides."""
    check(gpu, oracle, field(), "along the slab")


def test_the_field_from_outside_its_grid(gpu, oracle):
    check(gpu, oracle, field(look_from=(13.0, 2.0, 3.0), look_at=(0.0, 0.5, 0.0)), "from outside")


def test_a_small_pool_from_above_where_no_segment_needs_a_scan(gpu, oracle):
    check(gpu, oracle, small_pool_from_above(), "from above")


def test_a_tall_pool_where_hardly_a_segment_is_listable(gpu, oracle):
    check(gpu, oracle, tall_pool(), "tall pool")


@pytest.mark.parametrize("outliers", [MAX_OUTLIERS, MAX_OUTLIERS + 1])
def test_eight_outliers_have_cells_and_nine_scan(gpu, oracle, outliers):
    check(gpu, oracle, field(look_from=(3.0, 3.0, 12.0), look_at=(0.0, 0.5, 0.0), outliers=outliers), f"{outliers} outliers",
          has_cells=outliers <= MAX_OUTLIERS, precisions=(F32,))


def test_fewer_live_lanes_than_the_threshold_from_the_start(gpu, oracle):
    t = field()
    check(gpu, oracle, t, "8x4", cams=[camera(oracle, ((3.0, 2.0, 12.0), 40.0, 10.0), 8, 4)], width=8, height=4)


def test_a_shard(gpu, oracle):
    t = field(look_from=(3.0, 2.0, 12.0), look_at=(0.0, 0.5, 0.0))
    p = dist.shard_params(t.params(), 0, 8)
    rows = render.shard_row_indices(H, p.tile_rows, 0, 8)
    assert 0 < len(rows) < H and render.shard_rows(p) == len(rows)
    check(gpu, oracle, t, "rank 0 of 8", rows=rows, tile_rows=p.tile_rows, shard_index=0, shard_count=8)


def test_a_repadded_device_scene_keeps_its_cells(gpu, oracle):
    """The far camera's origin bound makes the scene rebuild its filter streams; the table hangs on the slots, which stay."""
    t = field()
    near, far = camera(oracle, ((3.0, 2.0, 12.0), 40.0, 10.0), W, H), camera(oracle, ((90.0, 30.0, 120.0), 6.0, 150.0), W, H)
    check(gpu, oracle, t, "re-padded", cams=[near, far, near], precisions=(F32,))


@pytest.mark.parametrize("prec", [F32, F64])
def test_a_progressive_handle_in_four_passes_ends_in_the_one_shot_frame(gpu, oracle, prec):
    t = field(look_from=(3.0, 2.0, 12.0), look_at=(0.0, 0.5, 0.0))
    t.samples_per_px = 32
    scene, cam = t.scene_desc(), t.camera_desc()
    p = params(t.params(), traversal=LINEAR, precision=prec, chunk_spp=8)
    ds = gpu.DeviceScene(scene)
    try:
        ds.set_cell_lists(ON)
        ds.set_primary_lists(P_ON)
        one_shot, seg = render_once(ds, cam, p)
        ref, ost = oracle.render_b(scene, cam, p)
        assert_images_equal(one_shot, ref, "one shot")
        assert seg == ost.segments
        pr = ds.progressive(cam, p)
        try:
            passes = 0
            while not pr.done:
                out = out_tensor(p)
                pr.step(0, out.data_ptr())
                passes += 1
            st = pr.stats()  # (waits for the last pass)
            assert passes == pr.n_chunks == 4
            assert_images_equal(out.cpu().numpy(), one_shot, "four passes")
            assert st.segments == seg
        finally:
            pr.close()
    finally:
        ds.close()


def _members(n):
    t = tracer.Tracer.init(W, 40.0, 10.0, 0.0, (0.0, 4.0, 14.0), (0.0, 0.0, 0.0), (0, 1, 0), seed=3)
    m = t.pool.add_diffuse(t.pool.add_solid_texture((0.5, 0.5, 0.5)), 0)
    rng = np.random.default_rng(n)
    t.pool.add_sphere((0.0, -1000.0, 0.0), 1000.0, int(m))
    for k in range(n):
        t.pool.add_sphere((k % 40 + 0.8 * rng.uniform(), 0.1, k // 40 + 0.8 * rng.uniform()), 0.1, int(m))
    return t


def test_autos_gate(gpu):
    for n, on in [(MIN_MEMBERS, True), (MIN_MEMBERS - 1, False)]:
        ds = gpu.DeviceScene(_members(n).scene_desc())
        try:
            assert ds.uses_cell_lists() == on, n
            ds.set_cell_lists(ON)
            assert ds.uses_cell_lists()
            ds.set_cell_lists(OFF)
            assert not ds.uses_cell_lists()
            ds.set_cell_lists(AUTO)
            assert ds.uses_cell_lists() == on
            with pytest.raises(capi.RayzHipError):
                ds.set_cell_lists(3)
        finally:
            ds.close()
