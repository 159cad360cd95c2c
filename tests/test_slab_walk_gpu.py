"""The walk on the device: the cells kernels resolve a segment whose box holds more than kMaxCells cells from the
cells its stretch crosses, column by column, as long as it crosses at most kWalkColumns columns.  `check` of test_slab_cells_gpu.py:
cells OFF and ON under the three scan forms, with and without primary lists, f32 and f64, each frame and its segments byte for byte
the oracle's and the BVH frame's.  Frames of at most 64x36 at 8 spp.  The product kernels carry no counters: test_slab_walk_cpu.py
runs the host mirror of the query on each scene's pixel-centre camera rays and shows which classes of ray (box, walk, over the column
cap) a scene's first segments alone hold at least a hundred of; the later segments scatter from there."""
import pytest

from rayz_amd import dist, render
from test_reuse_gpu import camera, out_tensor, params
from test_slab_cells_gpu import F32, H, LINEAR, ON, P_ON, W, _lattice, _tracer, check, field, render_once
from helpers import assert_images_equal

pytestmark = pytest.mark.gpu

WALK_COLUMNS = 12  # slab_cells.hpp: kWalkColumns


def lattice24(look_from, look_at, seed=211):
    """24 x 24 members about the origin on a ground, and a unit sphere: 578 hittables."""
    t, rng, mats = _tracer(seed, look_from, look_at)
    t.pool.add_sphere((0.0, -1000.0, 0.0), 1000.0, int(mats[1]))
    t.pool.add_sphere((-3.0, 1.0, -5.0), 1.0, int(mats[3]))
    _lattice(t, rng, mats, 24)
    return t


def strip(seed=212):
    """40 members long in z and 3 wide, seen end-on from just above the slab through a long lens: the stretches run 10 to 40 cells
    of the strip's length."""
    t, rng, mats = _tracer(seed, (0.3, 1.0, 23.0), (0.0, 0.0, -20.0), vfov=8.0)
    t.pool.add_sphere((0.0, -1000.0, 0.0), 1000.0, int(mats[1]))
    for a in range(3):
        for b in range(40):
            vy = float(rng.uniform(0.05, 0.5)) if (a + b) % 3 == 0 else 0.0
            t.pool.add_sphere((a - 1.5 + 0.9 * rng.uniform(), 0.2, b - 20.0 + 0.9 * rng.uniform()), 0.2, int(mats[(3 * b + a) % len(mats)]),
                              velocity=(0.0, vy, 0.0))
    return t


SCENES = {  # name: (the scene, the classes its camera rays hold a hundred of: the CPU test below)
    "along z": (lambda: lattice24((0.3, 0.45, 14.0), (0.3, 0.45, 0.0)), ("box", "walk")),
    "along the diagonal": (lambda: lattice24((11.0, 0.45, 11.5), (0.0, 0.45, 0.0)), ("box", "walk")),
    "from above": (lambda: lattice24((3.0, 2.0, 12.0), (0.0, 0.5, 0.0)), ("box", "walk")),
    "strip": (strip, ("walk", "over")),
    "field": (lambda: field(look_from=(3.0, 2.0, 12.0), look_at=(0.0, 0.5, 0.0)), ("box", "walk")),
}


@pytest.mark.parametrize("name", ["along z", "along the diagonal"])
def test_a_camera_at_slab_height(gpu, oracle, name):
    """Origins inside the slab, level stretches of every length along z (z is major) and along the diagonal (ties, both axes)."""
    check(gpu, oracle, SCENES[name][0](), name)


def test_long_descents_from_above_the_slab(gpu, oracle):
    check(gpu, oracle, SCENES["from above"][0](), "from above")


def test_a_strip_seen_end_on(gpu, oracle):
    """Walks of up to 40 columns: over the cap and under it side by side."""
    check(gpu, oracle, strip(), "strip")


def test_the_field_with_its_overflowed_cell_on_walked_stretches(gpu, oracle):
    check(gpu, oracle, SCENES["field"][0](), "field")


def test_fewer_live_lanes_than_the_threshold_long_and_short_mixed(gpu, oracle):
    t = lattice24((3.0, 2.0, 12.0), (0.0, 0.5, 0.0))
    check(gpu, oracle, t, "8x4", cams=[camera(oracle, ((3.0, 2.0, 12.0), 40.0, 10.0), 8, 4)], width=8, height=4)


def test_a_shard(gpu, oracle):
    t = lattice24((3.0, 2.0, 12.0), (0.0, 0.5, 0.0))
    p = dist.shard_params(t.params(), 0, 8)
    rows = render.shard_row_indices(H, p.tile_rows, 0, 8)
    assert 0 < len(rows) < H
    check(gpu, oracle, t, "rank 0 of 8", rows=rows, tile_rows=p.tile_rows, shard_index=0, shard_count=8)


def test_a_progressive_handle_in_four_passes_ends_in_the_one_shot_frame(gpu, oracle):
    t = lattice24((0.3, 0.45, 14.0), (0.3, 0.45, 0.0))
    t.samples_per_px = 32
    scene, cam = t.scene_desc(), t.camera_desc()
    p = params(t.params(), traversal=LINEAR, precision=F32, chunk_spp=8)
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
