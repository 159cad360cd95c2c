"""The BVH kernels on every layout their tree can take (tests/bvh_layout_scenes.py; tests/test_bvh_layouts_cpu.py is the CPU part):
several oversized hittables of every kind in the pre-walk of all three kernels (render, adaptive pass, query), the cap of eight, the
stop at kMinTree, a tree at its depth budget, and every place the walk can read a record from (an LDS top of 0, 1, 2 or 5 records
or the default, numbered by area or breadth-first, with and without peeling, both node formats).  Renders are held to oracle mode B
bit for bit, queries to the flat list field by field, to the mode-B brute force bit for bit and to the exact reference within its
own bounds.  Every scene first asserts, through the library's own builder, that it forms the layout it was built for."""
import numpy as np
import pytest
import torch

import bvh_layout_scenes as scenes
from helpers import assert_images_equal
from query_reference import TMIN, brute_force
from rayz_amd import capi, render, tracer
from test_query_exact_gpu import _both, _exact, _run, frame_rays
from test_query_gpu import check_against_oracle

pytestmark = pytest.mark.gpu

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR, BVH = capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH
FIELDS = render.QUERY_OUTPUTS
KNOBS = (capi.DEBUG_BVH_TOP, capi.DEBUG_BVH_TOP_ORDER, capi.DEBUG_BVH_PEEL, capi.DEBUG_BVH_NODES, capi.DEBUG_BVH_SPLIT)
TOPS = (0, 1, 2, 5, -1)  # records of the tree's top kept in LDS; -1: as many as fit


@pytest.fixture(scope="module")
def mirror(built, tmp_path_factory):
    return scenes.mirror_exe(str(tmp_path_factory.mktemp("bvh_layout")))


_BIG = {}


def peeled(mirror, tmp_path, name, t):
    """The scene's oversized hittables, after asserting its layout."""
    if name not in _BIG:
        sd = t.scene_desc()
        _BIG[name] = scenes.check_layout(name, sd, scenes.layout(mirror, sd, tmp_path / "scene.bin"))
    return _BIG[name]


_WANT = {}


def oracle_frame(oracle, key, t):
    """oracle.render_b of a scene's frame, once per (scene, precision)."""
    if key not in _WANT:
        _WANT[key] = oracle.render_b(t.scene_desc(), t.camera_desc(), t.params())
        _WANT[key][0].setflags(write=False)
    return _WANT[key]


def reset_knobs():
    for k in KNOBS:
        render.debug_set(k, -1)


# ---- a. renders ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [F32, F64])
@pytest.mark.parametrize("name", scenes.NAMES)
def test_render_equals_the_oracle(gpu, oracle, mirror, tmp_path, name, prec):
    t = scenes.make(name)
    big = peeled(mirror, tmp_path, name, t)
    t.set_gpu(precision=prec, traversal=BVH)
    sd, cam = t.scene_desc(), t.camera_desc()
    want, ost = oracle_frame(oracle, (name, prec), t)
    got, gst = gpu.render_host(sd, cam, t.params())
    assert_images_equal(got, want, f"{name} precision {prec} BVH")
    assert gst.segments == ost.segments and gst.node_tests > 0
    # the pre-walk counts its entries per segment: the device's own witness of what was kept out of the tree
    assert gst.sphere_tests >= len(big) * gst.segments
    t.set_gpu(traversal=LINEAR)
    flat, fst = gpu.render_host(sd, cam, t.params())
    assert_images_equal(flat, want, f"{name} precision {prec} flat list")
    assert fst.segments == ost.segments and fst.node_tests == 0


@pytest.mark.parametrize("prec", [F32, F64])
@pytest.mark.parametrize("name", ["mixed5", "nine"])
def test_render_in_both_node_formats_and_both_splits(gpu, oracle, mirror, tmp_path, name, prec):
    t = scenes.make(name)
    big = peeled(mirror, tmp_path, name, t)
    t.set_gpu(precision=prec, traversal=BVH)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    want, ost = oracle_frame(oracle, (name, prec), t)
    try:
        for split in (0, 1):
            for fmt in (1, 2):
                gpu.debug_set(capi.DEBUG_BVH_SPLIT, split)
                gpu.debug_set(capi.DEBUG_BVH_NODES, fmt)
                got, gst = gpu.render_host(sd, cam, p)  # (a fresh scene per call: the knobs act when the tree is built)
                assert_images_equal(got, want, f"{name} precision {prec} split {split} node format {fmt}")
                assert gst.segments == ost.segments and gst.sphere_tests >= len(big) * gst.segments
    finally:
        reset_knobs()


# ---- b. where the walk reads its records -----------------------------------------------------------------------------------------
def _source_scene(name):
    if name == "randomBouncing":  # 1,600 spheres and the ground: a tree far larger than any of the caps
        t = tracer.randomBouncing(64, -20, 20, seed=42)
        t.samples_per_px, t.max_bounces = 4, 10
        t.set_gpu(render_seed=9)
        return t
    return scenes.make(name)


@pytest.mark.parametrize("prec", [F32, F64])
@pytest.mark.parametrize("name", ["nine", "line600", "randomBouncing"])
def test_image_and_counts_do_not_depend_on_where_a_record_is_read(gpu, oracle, mirror, tmp_path, name, prec):
    """Every top cap x numbering x peel (x node format on `nine`) gives the oracle's image and segments.  Within one (peel, format)
    the tree and its padded boxes are the same and a lane's walk depends on its own ray only, so node_tests and sphere_tests are
    EQUAL across every cap and numbering: where a record is fetched from changes no count."""
    t = _source_scene(name)
    n_big = len(peeled(mirror, tmp_path, name, t)) if name != "randomBouncing" else 1
    t.set_gpu(precision=prec, traversal=BVH)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    want, ost = oracle_frame(oracle, (name, prec), t)
    counts = {}
    try:
        for fmt in ((1, 2) if name == "nine" else (-1,)):
            for peel in (0, 1):
                for top in TOPS:
                    for order in (0, 1):
                        gpu.debug_set(capi.DEBUG_BVH_NODES, fmt)
                        gpu.debug_set(capi.DEBUG_BVH_PEEL, peel)
                        gpu.debug_set(capi.DEBUG_BVH_TOP, top)
                        gpu.debug_set(capi.DEBUG_BVH_TOP_ORDER, order)
                        got, gst = gpu.render_host(sd, cam, p)
                        what = f"{name} precision {prec} format {fmt} peel {peel} top {top} order {order}"
                        assert_images_equal(got, want, what)
                        assert gst.segments == ost.segments, what
                        counts.setdefault((fmt, peel), {})[(top, order)] = (gst.node_tests, gst.sphere_tests)
    finally:
        reset_knobs()
    for (fmt, peel), seen in counts.items():
        assert len(seen) == 10 and len(set(seen.values())) == 1, (name, prec, fmt, peel, seen)
        node_tests, sphere_tests = next(iter(seen.values()))
        assert node_tests > 0 and sphere_tests >= (n_big if peel else 0) * ost.segments
        print(f"{name} precision {prec} format {fmt} peel {peel}: {node_tests} box tests, {sphere_tests} primitive tests, {ost.segments} segments")
    for fmt in {f for f, _ in counts}:  # PEEL = 0 walks the outliers' ancestors for every ray: more box tests, no pre-walk
        if n_big:
            assert next(iter(counts[(fmt, 0)].values()))[0] > next(iter(counts[(fmt, 1)].values()))[0]


@pytest.mark.parametrize("prec", [F32, F64])
@pytest.mark.parametrize("name", ["nine", "line600"])
def test_queries_do_not_depend_on_where_a_record_is_read(gpu, oracle, mirror, tmp_path, name, prec):
    """The query kernel under the same knobs: NEAREST is the flat list's answer in every field and ANY its index >= 0, whatever
    the top, its numbering, the peel and (on `nine`) the node format."""
    t = scenes.make(name)
    big = peeled(mirror, tmp_path, name, t)
    sd = t.scene_desc()
    rays, _ = scenes.query_rays(oracle, name, t, big, prec)
    ds = render.DeviceScene(sd)
    flat = _run(ds, rays, prec, LINEAR)
    ds.close()
    assert (flat["index"] >= 0).mean() > 0.4
    try:
        for fmt in ((1, 2) if name == "nine" else (-1,)):
            for peel in (0, 1):
                for top in TOPS:
                    for order in (0, 1):
                        gpu.debug_set(capi.DEBUG_BVH_NODES, fmt)
                        gpu.debug_set(capi.DEBUG_BVH_PEEL, peel)
                        gpu.debug_set(capi.DEBUG_BVH_TOP, top)
                        gpu.debug_set(capi.DEBUG_BVH_TOP_ORDER, order)
                        ds = render.DeviceScene(sd)  # (a fresh scene per setting: the knobs act when the buffers are built)
                        got = _run(ds, rays, prec, BVH)
                        hit = _run(ds, rays, prec, BVH, kind="any")["hit"]
                        ds.close()
                        for k in FIELDS:
                            assert np.array_equal(got[k], flat[k]), (name, prec, fmt, peel, top, order, k)
                        assert np.array_equal(hit, (flat["index"] >= 0).astype(np.uint8)), (name, prec, fmt, peel, top, order)
    finally:
        reset_knobs()


# ---- c. queries ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [F32, F64])
@pytest.mark.parametrize("name", scenes.QUERY_NAMES)
def test_queries_held_to_the_exact_reference(gpu, oracle, mirror, tmp_path, name, prec):
    t = scenes.make(name)
    big = peeled(mirror, tmp_path, name, t)
    sd = t.scene_desc()
    rays, where = scenes.query_rays(oracle, name, t, big, prec)
    ds = render.DeviceScene(sd)
    got = _both(ds, rays, prec)  # NEAREST: BVH == flat list in every field; ANY == index >= 0 through both
    ds.close()
    s = _exact(sd, rays, got, prec, what=("bvh layout", name, prec))
    assert s["unambiguous"] >= 0.8
    want = brute_force(oracle, sd, rays, TMIN, prec)
    check_against_oracle(oracle, sd, want, got, prec)
    scenes.check_designed_parts(name, sd, big, rays, where, got["index"].astype(np.int64), oracle, prec)
    for i in big:  # every oversized hittable is somebody's nearest hit
        assert (got["index"] == i).any(), (name, i)
    if big:
        # two whole waves in which every lane meets an oversized hittable in the pre-walk and a nearer sphere in the walk: ANY is
        # done before the walk starts (no box is tested), NEAREST has to walk on to find the nearer one
        w = where["cluster_then_outlier"]
        ds = render.DeviceScene(sd)
        dt = torch.float64 if prec == F64 else torch.float32
        part = torch.tensor(rays[w], dtype=dt, device="cuda")
        hit = ds.query(part, tmin=TMIN, kind="any", traversal=BVH)
        any_st = ds.query_sync()
        near = ds.query(part, tmin=TMIN, kind="nearest", traversal=BVH)
        near_st = ds.query_sync()
        index = near.index.cpu().numpy()
        assert hit.hit.cpu().numpy().all() and np.array_equal(index, got["index"][w])
        ds.close()
        assert any_st.node_tests == 0 and any_st.sphere_tests == 128 * len(big)
        assert near_st.node_tests > 0 and near_st.sphere_tests > 128 * len(big)


@pytest.mark.parametrize("prec", [F32, F64])
def test_camera_form_equals_the_batch_form(gpu, oracle, mirror, tmp_path, prec):
    name = "nine"
    t = scenes.make(name)
    peeled(mirror, tmp_path, name, t)
    sd, cam = t.scene_desc(), t.camera_desc()
    p = t.params()
    p.precision, p.tmin, p.traversal = prec, TMIN, BVH
    ds = render.DeviceScene(sd)
    g = ds.gbuffer(cam, p)
    ds.query_sync()
    frame = {k: getattr(g, k).cpu().numpy() for k in FIELDS}
    batch = _run(ds, frame_rays(oracle, cam, p.width, p.height, prec), prec, BVH)
    ds.close()
    assert (frame["index"] >= 0).mean() > 0.5
    for k in FIELDS:
        assert np.array_equal(frame[k].reshape(batch[k].shape), batch[k]), k


# ---- d. adaptive passes: the third text of the pre-walk --------------------------------------------------------------------------
def _params(base, **kw):
    p = capi.RenderParams.from_buffer_copy(bytes(base))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _out(p):
    out = torch.full((render.shard_rows(p), p.width, 3), float("nan"), dtype=torch.float64 if p.precision == F64 else torch.float32,
                     device="cuda")
    torch.cuda.synchronize()
    return out


def _adaptive(ds, cam, p, rel_error, min_chunks, min_samples):
    pr = ds.progressive(cam, p, adaptive=True, min_chunks=min_chunks)
    try:
        out = _out(p)
        while True:
            sm = pr.adaptive_step(rel_error=rel_error, min_samples=min_samples, out=out)
            if sm.active == 0 or pr.done:
                break
        return out.cpu().numpy(), pr.frozen_at().cpu().numpy(), pr.sample_counts().cpu().numpy(), pr.stats()
    finally:
        pr.close()


def _plain(ds, cam, p, min_samples):
    """A plain tracked handle over the same boundaries: {chunks_done: (preview, rel2)}."""
    pr = ds.progressive(cam, p, track_noise=True)
    seen = {}
    try:
        while not pr.done:
            out = _out(p)
            pr.step(min_samples, out.data_ptr())
            _, _, rel2 = pr.noise(rel2=True)
            seen[pr.chunks_done] = (out.cpu().numpy(), rel2.cpu().numpy())
        return seen
    finally:
        pr.close()


# rel_error at which about half of each scene's pixels freeze before the schedule ends (squares exact in f32: rel2's single
# rounding to f32 cannot cross them)
ADAPTIVE_REL_ERROR = {"mixed5": 0.25, "nine": 0.5}


def _first_pass(plain, tau2, shape):
    """The first boundary (a pass end >= min_chunks 2) at which a pixel's estimate passes, 0 if none does."""
    first = np.zeros(shape, dtype=np.int64)
    for k in sorted(plain, reverse=True):
        first[plain[k][1] <= tau2] = k
    return first


@pytest.mark.parametrize("prec", [F32, F64])
@pytest.mark.parametrize("name", ["mixed5", "nine"])
def test_adaptive_passes_through_the_bvh(gpu, oracle, mirror, tmp_path, name, prec):
    """8 spp in chunks of 1, a pass per 2 samples, through adaptive_pass_kernel_bvh.  Where no pixel can freeze the frame is the
    one-shot frame bit for bit, and so the oracle's; at rel_error 1e-9 only pixels whose estimate is exactly 0 freeze and every
    other pixel is the oracle's.  With about half the pixels freezing on the way, every pixel is what tests/adaptive_ref.py
    states for it: frozen at the first boundary (>= min_chunks) at which its estimate passes, it holds the plain handle's
    preview at that boundary and that boundary's sample count; never frozen, it holds the one-shot pixel.  (adaptive_ref.run
    itself takes chunk sums, which a traced frame does not expose: its statement is applied through plain handles stepped over
    the same boundaries, as tests/test_adaptive_gpu.py does.)"""
    t = scenes.make(name)
    big = peeled(mirror, tmp_path, name, t)
    t.set_gpu(precision=prec, traversal=BVH, tmin=1e-3 if prec == F32 else 1e-10)
    sd, cam = t.scene_desc(), t.camera_desc()
    p = _params(t.params(), chunk_spp=1)
    assert p.samples_per_px == 8
    want, ost = oracle.render_b(sd, cam, p)
    rel = ADAPTIVE_REL_ERROR[name]
    ds = render.DeviceScene(sd)
    try:
        one_shot = _out(p)
        ds.render_into(cam, p, one_shot.data_ptr())
        ds.sync()
        one_shot = one_shot.cpu().numpy()
        assert_images_equal(one_shot, want, f"{name} one-shot, chunks of 1")
        plain = _plain(ds, cam, p, 2)
        assert sorted(plain) == [2, 4, 6, 8]
        frame, frozen, counts, st = _adaptive(ds, cam, p, 1e-9, 9, 2)  # min_chunks beyond the schedule: nothing can freeze
        assert (frozen == 0).all() and (counts == 8).all() and st.segments == ost.segments
        assert st.sphere_tests >= len(big) * st.segments
        assert_images_equal(frame, want, f"{name} adaptive, nothing frozen")
        frame, frozen, counts, st = _adaptive(ds, cam, p, 1e-9, 2, 2)  # only an estimate of exactly 0 passes (black pixels)
        assert (frozen == _first_pass(plain, np.float32(0.0), frozen.shape)).all()
        never = frozen == 0
        assert never.mean() > 0.25  # (in the room of `nine` more than half the pixels are black in their first two samples)
        assert_images_equal(frame[never], want[never], f"{name} adaptive at rel_error 1e-9")
        frame, frozen, counts, st = _adaptive(ds, cam, p, rel, 2, 2)  # about half the pixels freeze on the way
    finally:
        ds.close()
    tau2 = np.float32(rel * rel)
    assert float(tau2) == rel * rel
    first = _first_pass(plain, tau2, frozen.shape)
    assert (frozen == first).all(), f"frozen_at differs at {np.argwhere(frozen != first)[:4].tolist()}"
    early = np.count_nonzero((first != 0) & (first < 8)) / first.size
    print(f"{name} precision {prec}: {early:.3f} of the pixels freeze before the end, {np.mean(first == 0):.3f} never, "
          f"{np.mean(first == 2):.3f} at the first chance")
    assert 0.25 <= early <= 0.75 and len(np.unique(first)) >= 4  # about half, and not all in one pass
    expect = one_shot.copy()
    for k in sorted(plain):
        expect[first == k] = plain[k][0][first == k]
    assert_images_equal(frame, expect, f"{name} adaptive: frozen pixels vs plain previews, the rest vs the one-shot frame")
    n_i = np.where(first != 0, first, 8)
    assert (counts == n_i).all() and st.primary_rays == int(n_i.sum())
    assert (frame != one_shot).any()  # the freezing is visible in the frame
