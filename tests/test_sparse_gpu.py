"""Sparse renders on the GPU (rayz_hip_scene_render_pixels, `DeviceScene.render_pixels`): every listed pixel is
the whole frame's pixel bit for bit — whatever the list's order, length and duplicates, through the flat list and the BVH, in f32
and f64, on a shard, scattered by `dest`, and cycled as lattices — its variance is a tracked progressive handle's, its counters
are its own, and a list with an entry out of range is refused before anything is written."""
import functools

import numpy as np
import pytest
import torch

from rayz_amd import capi, render, tracer

pytestmark = pytest.mark.gpu

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR, BVH = capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH
ALL = 0xFFFFFFFF
SPP, CHUNK, BOUNCES = 12, 4, 4
CONFIGS = [(trav, prec) for trav in (LINEAR, BVH) for prec in (F32, F64)]
IDS = [f"{'bvh' if trav == BVH else 'flat'}-{'f64' if prec == F64 else 'f32'}" for trav, prec in CONFIGS]
SIZES = [(24, 16), (20, 12)]  # (width not a multiple of 8: 20)


def ibits(t):
    return t.contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def same(got, want, what):
    bad = (ibits(got) != ibits(want)).nonzero()
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.numel()} values differ, first at {bad[:4].tolist()}"


def params(base, **kw):
    p = capi.RenderParams.from_buffer_copy(bytes(base))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def nan_frame(shape, dtype):
    """A frame of one NaN pattern that no render produces: a slot that keeps it was not written."""
    if dtype == torch.float64:
        t = torch.full(shape, 0x7FF8000000C0FFEE, dtype=torch.int64, device="cuda").view(torch.float64)
    else:
        t = torch.full(shape, 0x7FC0BEEF, dtype=torch.int32, device="cuda").view(torch.float32)
    torch.cuda.synchronize()
    return t


class Setup:
    """A small scene on the device, the frame's camera and params, and the whole frame rendered once (left unchanged)."""

    def __init__(self, trav, prec, width, height, **kw):
        # the flat list: three spheres; the BVH: ~485 spheres, every material, checker texture and motion blur
        self.t = tracer.threeSpheres(width, seed=1) if trav == LINEAR else tracer.randomBouncing(width, seed=7)
        self.t.samples_per_px, self.t.max_bounces = SPP, BOUNCES
        self.t.set_gpu(render_seed=11, precision=prec, traversal=trav, chunk_spp=CHUNK, tmin=1e-3 if prec == F32 else 1e-10)
        self.scene, self.cam = self.t.scene_desc(), self.t.camera_desc()
        self.p = params(self.t.params(), height=height, **kw)  # (the camera's rays exist for any row: the frame is well defined)
        self.dtype = torch.float64 if prec == F64 else torch.float32
        self.ds = render.DeviceScene(self.scene)
        self.frame = self.whole(self.p)

    def whole(self, p):
        out = nan_frame((render.shard_rows(p), p.width, 3), self.dtype)
        self.ds.render_into(self.cam, p, out.data_ptr())
        self.ds.sync()
        return out


@functools.lru_cache(maxsize=None)
def setup(trav, prec, width, height):
    return Setup(trav, prec, width, height)


def at_rows(pixels):
    """The entries as an index into a (pixels, 3) view of a frame."""
    return torch.as_tensor(np.ascontiguousarray(pixels, dtype=np.int64), device="cuda")


def listed(pixels):
    t = torch.as_tensor(np.ascontiguousarray(pixels, dtype=np.int32), device="cuda")
    torch.cuda.synchronize()
    return t


# ---- the whole frame, listed ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("trav,prec", CONFIGS, ids=IDS)
def test_listed_pixels_are_the_frames_pixels(gpu, trav, prec, size):
    s = setup(trav, prec, *size)
    n = size[0] * size[1]
    flat = s.frame.reshape(n, 3)
    rng = np.random.default_rng(3)
    lists = {"row-major": np.arange(n), "reversed": np.arange(n)[::-1], "permuted with duplicates": rng.integers(0, n, size=n + 37)}
    for m in (1, 63, 64, 65, 257):
        lists[f"{m} entries"] = rng.integers(0, n, size=m)
    for what, pixels in lists.items():
        got = s.ds.render_pixels(s.cam, s.p, listed(pixels))
        st = s.ds.sync()
        assert tuple(got.shape) == (len(pixels), 3) and got.dtype == s.dtype
        same(got, flat[at_rows(pixels)], what)
        assert st.primary_rays == len(pixels) * SPP and st.segments >= st.primary_rays and st.kernel_ms > 0, what
        assert (st.node_tests > 0) == (trav == BVH) and st.sphere_tests > 0
    same(s.frame, s.whole(s.p), "the frame, rendered again after the sparse renders")


@pytest.mark.parametrize("trav,prec", CONFIGS, ids=IDS)
def test_eight_pixels_equal_the_oracle(gpu, oracle, trav, prec):
    s = setup(trav, prec, 24, 16)
    pixels = np.array([0, 23, 24 * 15, 24 * 16 - 1, 100, 101, 211, 100])  # the corners, neighbours, a duplicate
    want, ost = oracle.render_b(s.scene, s.cam, s.p, pixels=pixels)
    got = s.ds.render_pixels(s.cam, s.p, listed(pixels))
    st = s.ds.sync()
    same(got, torch.as_tensor(want, device="cuda"), "against mode B")
    assert st.segments == ost.segments and st.primary_rays == ost.primary_rays == 8 * SPP


# ---- scatter ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trav,prec", CONFIGS, ids=IDS)
def test_dest_scatters_and_leaves_every_other_slot(gpu, trav, prec):
    s = setup(trav, prec, 20, 12)
    n = 20 * 12
    rng = np.random.default_rng(4)
    pixels = rng.permutation(n)[:97]
    dest = rng.permutation(n + 50)[:97]  # an output larger than the frame, every slot named at most once
    out, var = nan_frame((n + 50, 3), s.dtype), nan_frame((n + 50, 3), torch.float32)
    before, before_var = out.clone(), var.clone()
    got, got_var = s.ds.render_pixels(s.cam, s.p, listed(pixels), dest=listed(dest), out=out, var=var)
    s.ds.sync()
    assert got is out and got_var is var
    at = at_rows(dest)
    same(out[at], s.frame.reshape(n, 3)[at_rows(pixels)], "the named slots")
    rest = torch.ones(n + 50, dtype=torch.bool, device="cuda")
    rest[at] = False
    same(out[rest], before[rest], "the colour slots nobody named")
    same(var[rest], before_var[rest], "the variance slots nobody named")
    assert torch.isfinite(var[at]).all() and (var[at] >= 0).all()
    # two entries, one slot: one of them stays, and the same pixel gives the same bits either way
    out2 = nan_frame((3, 3), s.dtype)
    s.ds.render_pixels(s.cam, s.p, listed([5, 5, 9]), dest=listed([1, 1, 1]), out=out2)
    s.ds.sync()
    flat = s.frame.reshape(n, 3)
    assert any((ibits(out2[1]) == ibits(flat[k])).all() for k in (5, 9))
    same(out2[[0, 2]], nan_frame((2, 3), s.dtype), "the slots beside the shared one")


# ---- shards ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trav,prec", CONFIGS, ids=IDS)
def test_a_shards_local_pixels(gpu, trav, prec):
    s = setup(trav, prec, 24, 16)
    p = params(s.p, shard_count=2, tile_rows=4, shard_index=1)
    rows = render.shard_rows(p)
    assert rows == 8
    shard = s.whole(p)
    same(shard, s.frame[render.shard_row_indices(16, 4, 1, 2)], "the shard is the frame's rows 4-7 and 12-15")
    pixels = np.random.default_rng(5).permutation(rows * 24)
    got = s.ds.render_pixels(s.cam, p, listed(pixels))
    assert s.ds.sync().primary_rays == rows * 24 * SPP
    same(got, shard.reshape(rows * 24, 3)[at_rows(pixels)], "local indices of the shard")
    with pytest.raises(capi.RayzHipError, match="outside the shard"):  # a pixel of the frame that is none of the shard
        s.ds.render_pixels(s.cam, p, listed([rows * 24]))


# ---- the variance ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spp,bounces", [(SPP, BOUNCES), (CHUNK, BOUNCES), (SPP, 0)], ids=["three-chunks", "one-chunk", "no-bounces"])
@pytest.mark.parametrize("trav,prec", CONFIGS, ids=IDS)
def test_variance_is_a_tracked_handles(gpu, trav, prec, spp, bounces):
    s = setup(trav, prec, 20, 12)
    p = params(s.p, samples_per_px=spp, max_bounces=bounces)
    n = 20 * 12
    pr = s.ds.progressive(s.cam, p, track_noise=True)
    try:
        frame = nan_frame((12, 20, 3), s.dtype)
        pr.step(ALL, frame.data_ptr())
        want_var = pr.noise_rgb()
        pr.stats()
        assert pr.done
        pixels = np.random.default_rng(6).integers(0, n, size=150)
        at = at_rows(pixels)
        got, var = s.ds.render_pixels(s.cam, p, listed(pixels), var=True)
        st = s.ds.sync()
        same(got, frame.reshape(n, 3)[at], "colour")
        same(var, want_var.reshape(n, 3)[at], "variance")
        assert st.primary_rays == 150 * spp
        if spp == CHUNK:
            assert torch.isposinf(var).all()
        elif bounces == 0:
            assert (ibits(got) == 0).all() and (ibits(var) == 0).all()  # +0
        else:
            assert torch.isfinite(var).all() and (var > 0).any()
    finally:
        pr.close()


# ---- refusal ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("trav,prec", [(LINEAR, F32), (BVH, F64)], ids=["flat-f32", "bvh-f64"])
def test_an_entry_out_of_range_is_refused_with_nothing_written(gpu, trav, prec):
    """The validation path: the entry is compared on the device and never indexes anything."""
    s = setup(trav, prec, 24, 16)
    n = 24 * 16
    out, var = nan_frame((1, 3), s.dtype), nan_frame((1, 3), torch.float32)
    with pytest.raises(capi.RayzHipError, match=r"status -1\).*1 of 1 entries"):
        s.ds.render_pixels(s.cam, s.p, listed([n]), out=out, var=var)  # ONE entry, equal to the shard's pixel count
    torch.cuda.synchronize()
    same(out, nan_frame((1, 3), s.dtype), "the output of the refused call")
    same(var, nan_frame((1, 3), torch.float32), "the variance of the refused call")
    frame = nan_frame((n, 3), s.dtype)
    with pytest.raises(capi.RayzHipError, match=r"status -1\).*1 of 3 entries"):
        s.ds.render_pixels(s.cam, s.p, listed([0, 1, 2]), dest=listed([0, n, 2]), out=frame)  # a slot equal to dest_pixels
    torch.cuda.synchronize()
    same(frame, nan_frame((n, 3), s.dtype), "the frame of the refused call")
    with pytest.raises(capi.RayzHipError, match="status -1"):
        s.ds.render_pixels(s.cam, s.p, listed([0, 1]), out=nan_frame((3, 3), s.dtype))  # no dest: one slot per entry
    got = s.ds.render_pixels(s.cam, s.p, listed([n - 1]))  # .. and the scene renders on
    s.ds.sync()
    same(got, s.frame.reshape(n, 3)[n - 1:], "the last pixel, after the refusals")
    empty = s.ds.render_pixels(s.cam, s.p, listed([]))
    assert tuple(empty.shape) == (0, 3)


# ---- lattices: the phases of a still camera rebuild the frame ----------------------------------------------------------------------
@pytest.mark.parametrize("f", [2, 3, 4])
@pytest.mark.parametrize("trav,prec", CONFIGS, ids=IDS)
def test_the_phase_cycle_is_the_one_shot_frame(gpu, trav, prec, f):
    s = setup(trav, prec, 24, 24)
    out = nan_frame((24, 24, 3), s.dtype)
    lo_w = 24 // f
    for k, phase in enumerate(render.phase_sequence(f)):
        pixels, dest = render.lattice_pixels(24, 24, f, phase, order=("rows", "tiles")[k % 2], device="cuda")
        torch.cuda.synchronize()
        if k == 0:  # the lattice frame itself: the frame's pixels [py::f, px::f]
            lo = s.ds.render_pixels(s.cam, s.p, pixels, dest=dest, out=nan_frame((lo_w, lo_w, 3), s.dtype))
            s.ds.sync()
            same(lo, s.frame[phase[1]::f, phase[0]::f], "the lattice frame")
        s.ds.render_pixels(s.cam, s.p, pixels, dest=pixels, out=out)
        assert s.ds.sync().primary_rays == lo_w * lo_w * SPP
    same(out, s.frame, f"f = {f}: every phase scattered to its own pixels")
