"""The flat list's other two consumers on every stream layout the form kernels render (tests/flat_layout_scenes.py;
tests/test_flat_layouts_cpu.py is the CPU part): query_kernel<float> and query_kernel<double>, and the flat adaptive_pass_kernel.
Both inline the scan text of trace_kernel_flat.hpp, always in the XZ basis and without the set loop, so they read every run,
remainder, bucket and slot the layouts make, but with a state around the scan the render kernels do not have: a finite tmax as
the first tbest, lanes past the batch under full EXEC, work items from an active list over chunk windows with c0 > 0, and the
query path's own origin bound and re-pad.  Queries are held to the BVH field by field, to the mode-B brute force bit for bit and
to the exact reference within its own bounds; adaptive frames to the oracle and to plain handles stepped over the same boundaries
under every forced scan form (windows with c0 > 0 through flat_xy_kernel and flat_one_radius_kernel).  Every scene first asserts,
through the CPU mirrors, that it forms the layout it was built for.  pytest -s prints each scene's unambiguous share and the
rel_error its adaptive test chose."""
import numpy as np
import pytest
import torch

import flat_layout_scenes as scenes
from helpers import assert_images_equal
from query_reference import TMIN, brute_force
from rayz_amd import capi, render
from test_bvh_layouts_gpu import _adaptive, _first_pass, _out, _params, _plain
from test_one_radius import omirror  # noqa: F401  (a fixture)
from test_plane_runs import mirror  # noqa: F401  (a fixture)
from test_query_exact_gpu import _both, _capi_query, _exact, _outputs, _run, _untouched, frame_rays
from test_query_gpu import check_against_oracle
from test_speed_buckets import bmirror  # noqa: F401  (a fixture)

pytestmark = pytest.mark.gpu

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR, BVH = capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH
AUTO, XZ, XY, ONE = capi.SCAN_FORM_AUTO, capi.SCAN_FORM_XZ, capi.SCAN_FORM_XY, capi.SCAN_FORM_ONE_RADIUS
FIELDS = render.QUERY_OUTPUTS

_LAY, _FRAMES = {}, {}


def layout_of(name, t, exes, tmp_path):
    """The scene's units, after asserting its layout (once per scene)."""
    if name not in _LAY:
        _LAY[name] = scenes.check_layout(name, t, exes, tmp_path)
    return _LAY[name]


def frame_setup(name, prec):
    """(tracer, scene, camera, params) of the scene's frame through the flat list: 8 spp in chunks of 1."""
    t = scenes.make(name)
    t.set_gpu(precision=prec, traversal=LINEAR, tmin=1e-3 if prec == F32 else 1e-10)
    p = _params(t.params(), chunk_spp=1)
    assert p.samples_per_px == 8
    return t, t.scene_desc(), scenes.camera(name, t), p


def one_shot(ds, cam, p):
    out = _out(p)
    ds.render_into(cam, p, out.data_ptr())
    st = ds.sync()
    return out.cpu().numpy(), st


def same_fields(a, b, what):
    for k in FIELDS:
        assert np.array_equal(a[k], b[k]), (what, k, int((a[k] != b[k]).sum()))


# ---- a. queries ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [F32, F64])
@pytest.mark.parametrize("name", scenes.QUERY_NAMES)
def test_queries_on_every_layout(gpu, oracle, mirror, bmirror, omirror, tmp_path, name, prec):
    """One DeviceScene through the near batch, the far rim part (origins 20,000 units out: the query path re-pads every section
    for its larger origin bound) and the near batch again; then under every forced scan form, and around a ONE_RADIUS render."""
    t, sd, cam, p = frame_setup(name, prec)
    lay = layout_of(name, t, (mirror, bmirror, omirror), tmp_path)
    rays, where = scenes.query_rays(oracle, name, t, lay, prec)
    cut = where["far"].start
    near, far = rays[:cut], rays[cut:]
    want_near = brute_force(oracle, sd, near, TMIN, prec)
    ds = render.DeviceScene(sd)
    try:
        first = _both(ds, near, prec)  # NEAREST: flat list == BVH in every field; ANY == index >= 0 through both
        check_against_oracle(oracle, sd, want_near, first, prec)
        index = first["index"].astype(np.int64)
        if len(far):
            want_far = brute_force(oracle, sd, far, TMIN, prec)
            got_far = _both(ds, far, prec)
            missed = (want_far[0] >= 0) & (got_far["index"] < 0)
            assert not missed.any(), f"{name}: {int(missed.sum())} far grazing hits missed"
            check_against_oracle(oracle, sd, want_far, got_far, prec)
            index = np.concatenate([index, got_far["index"].astype(np.int64)])
            again = _run(ds, near, prec, LINEAR)
            same_fields(again, first, "near again after the far batch")
        facts = scenes.check_designed_parts(name, sd, lay, rays, where, index, oracle, prec)
        keep = scenes.without_ties(where, len(rays))[:cut]
        s = _exact(sd, near[keep], {k: v[keep] for k, v in first.items()}, prec, what=("flat layout", name, prec))
        print(f"{name} precision {prec}: {len(rays)} rays, hit share {facts['hit_share']:.3f}, unambiguous {s['unambiguous']:.3f}")
        assert s["unambiguous"] >= 0.8
        # partial waves: the lanes past the batch re-trace its last ray under full EXEC and must write nothing
        if "row" in where:
            part = near[where["row"]]
            whole = _run(ds, part, prec, LINEAR)
            same_fields(whole, {k: first[k][where["row"]] for k in FIELDS}, "the row part on its own")
            dt = torch.float64 if prec == F64 else torch.float32
            part_t = torch.tensor(part, dtype=dt, device="cuda")
            for n in (1, 63, 65, len(part) - 1):
                got = _capi_query(ds, part_t, n, capi.QUERY_NEAREST, LINEAR, prec, _outputs(n + 1, dt), FIELDS + ("hit",))
                for k in FIELDS:
                    assert np.array_equal(got[k][:n].numpy().reshape(whole[k][:n].shape), whole[k][:n]), (n, k)
                    assert _untouched(got[k][n:]), (n, k, "written past the batch")
                assert np.array_equal(got["hit"][:n, 0].numpy(), (whole["index"][:n] >= 0).astype(np.uint8)) and _untouched(got["hit"][n:])
        # the scene's scan form is the render kernels' business: no query field depends on it
        for form in (XZ, XY, ONE):
            ds.scan_form = form
            assert ds.scan_form == form
            same_fields(_run(ds, near, prec, LINEAR), first, f"scan form {form}")
        # .. and a flat render under ONE_RADIUS between two queries changes neither the queries nor the frame
        want, ost = oracle.render_b(sd, cam, p)
        frame, st = one_shot(ds, cam, p)
        assert_images_equal(frame, want, f"{name} precision {prec}: ONE_RADIUS frame between two queries")
        assert st.segments == ost.segments
        same_fields(_run(ds, near, prec, LINEAR), first, "after a ONE_RADIUS render")
        frame2, _ = one_shot(ds, cam, p)
        assert np.array_equal(frame2, frame)
        frame.setflags(write=False)
        _FRAMES[(name, prec)] = frame
    finally:
        ds.close()


# ---- b. the camera form ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [F32, F64])
@pytest.mark.parametrize("name", scenes.CAMERA_NAMES)
def test_camera_form_equals_the_batch_form(gpu, oracle, mirror, bmirror, omirror, tmp_path, name, prec):
    """tests/test_query_gpu.py: test_camera_form, through the flat list: the G-buffer is the batch query on every pixel's ray,
    and its three shards with tile_rows = 4 are the whole frame's rows."""
    t = scenes.make(name)
    layout_of(name, t, (mirror, bmirror, omirror), tmp_path)
    sd, cam = t.scene_desc(), scenes.camera(name, t)
    p = t.params()
    p.precision, p.tmin, p.traversal = prec, TMIN, LINEAR
    ds = render.DeviceScene(sd)
    try:
        g = ds.gbuffer(cam, p)
        ds.query_sync()
        whole = {k: getattr(g, k).cpu().numpy() for k in FIELDS}
        batch = _run(ds, frame_rays(oracle, cam, p.width, p.height, prec), prec, LINEAR)
        assert 0.3 < (whole["index"] >= 0).mean()
        for k in FIELDS:
            assert np.array_equal(whole[k].reshape(batch[k].shape), batch[k]), k
        for si in range(3):
            ps = capi.RenderParams.from_buffer_copy(p)
            ps.shard_index, ps.shard_count, ps.tile_rows = si, 3, 4
            gs = ds.gbuffer(cam, ps)
            ds.query_sync()
            rows = render.shard_row_indices(p.height, 4, si, 3)
            for k in FIELDS:
                assert np.array_equal(getattr(gs, k).cpu().numpy(), whole[k][rows]), (si, k)
    finally:
        ds.close()


# ---- c. adaptive passes through the flat list ------------------------------------------------------------------------------------------
def mid_rel_error(rel2_at_4):
    """The 2^-k whose square is nearest (in ratio) the median of the plain handle's rel2 at boundary 4: chosen from trace_kernel's
    estimates, not from the kernel under test; its square is exact in f32."""
    med = float(np.median(np.nan_to_num(rel2_at_4.astype(np.float64), nan=np.inf)))
    assert 0 < med < np.inf, med
    k = int(np.round(-0.5 * np.log2(med)))
    assert 0 <= k <= 60
    return 2.0 ** -k


@pytest.mark.parametrize("prec", [F32, F64])
@pytest.mark.parametrize("name", scenes.ADAPTIVE_NAMES)
def test_adaptive_passes_through_the_flat_list(gpu, oracle, mirror, bmirror, omirror, tmp_path, name, prec):
    """The statement of tests/test_bvh_layouts_gpu.py: test_adaptive_passes_through_the_bvh, through the flat adaptive_pass_kernel:
    8 spp in chunks of 1, a pass per 2 samples.  Nothing can freeze: the one-shot frame and the oracle's, bit for bit, equal
    segments.  rel_error 1e-9: only exact-zero estimates freeze, the rest is the oracle's.  A mid rel_error: every frozen pixel is
    the plain handle's preview at its first passing boundary, counts and primary_rays agree.  The plain handles run once per forced
    scan form (XZ, XY, ONE_RADIUS: chunk windows with c0 > 0 through all three form kernels) and give the same previews at every
    boundary; one more changes its form between steps and ends on the one-shot frame."""
    t, sd, cam, p = frame_setup(name, prec)
    layout_of(name, t, (mirror, bmirror, omirror), tmp_path)
    want, ost = oracle.render_b(sd, cam, p)
    ds = render.DeviceScene(sd)
    try:
        shot, st = one_shot(ds, cam, p)
        assert_images_equal(shot, want, f"{name} one-shot, chunks of 1")
        assert st.segments == ost.segments and st.node_tests == 0
        plains = {}
        for form in (XZ, XY, ONE):
            ds.scan_form = form
            plains[form] = _plain(ds, cam, p, 2)
            assert sorted(plains[form]) == [2, 4, 6, 8]
        plain = plains[XZ]
        for form in (XY, ONE):
            for k in plain:
                assert np.array_equal(plains[form][k][0], plain[k][0]), (name, prec, form, k, "preview")
                assert np.array_equal(plains[form][k][1], plain[k][1], equal_nan=True), (name, prec, form, k, "rel2")
        assert_images_equal(plain[8][0], shot, f"{name}: the plain handle's last frame vs the one-shot frame")
        kept = _FRAMES.get((name, prec))  # the ONE_RADIUS one-shot frame test_queries_on_every_layout rendered between two queries
        if kept is not None:
            assert_images_equal(plains[ONE][8][0], kept, f"{name}: windowed vs one-shot under ONE_RADIUS")
        pr = ds.progressive(cam, p)  # a handle whose form changes between steps
        try:
            for form in (ONE, XZ, XY, ONE):
                ds.scan_form = form
                out = _out(p)
                pr.step(2, out.data_ptr())
                pr.stats()
            assert pr.done
            assert_images_equal(out.cpu().numpy(), shot, f"{name}: a handle stepped under changing forms")
        finally:
            pr.close()
        rel = mid_rel_error(plain[4][1])
        results = {}
        for form in (AUTO, XZ, ONE):  # the adaptive frame does not depend on the scene's scan form
            ds.scan_form = form
            frame, frozen, counts, st = _adaptive(ds, cam, p, 1e-9, 9, 2)  # min_chunks beyond the schedule: nothing can freeze
            assert (frozen == 0).all() and (counts == 8).all() and st.segments == ost.segments and st.node_tests == 0
            assert_images_equal(frame, want, f"{name} adaptive, nothing frozen, form {form}")
            results[form] = _adaptive(ds, cam, p, rel, 2, 2)
        ds.scan_form = AUTO
        for form in (XZ, ONE):
            for a, b in zip(results[form][:3], results[AUTO][:3]):
                assert np.array_equal(a, b), (name, prec, form)
            assert results[form][3].primary_rays == results[AUTO][3].primary_rays
        frame, frozen, counts, st = _adaptive(ds, cam, p, 1e-9, 2, 2)  # only an estimate of exactly 0 passes (black pixels)
        assert (frozen == _first_pass(plain, np.float32(0.0), frozen.shape)).all()
        never = frozen == 0
        assert never.any()
        assert_images_equal(frame[never], want[never], f"{name} adaptive at rel_error 1e-9")
        frame, frozen, counts, st = results[AUTO]  # about half the pixels freeze on the way
    finally:
        ds.close()
    tau2 = np.float32(rel * rel)
    assert float(tau2) == rel * rel
    first = _first_pass(plain, tau2, frozen.shape)
    assert (frozen == first).all(), f"frozen_at differs at {np.argwhere(frozen != first)[:4].tolist()}"
    early = np.count_nonzero((first != 0) & (first < 8)) / first.size
    print(f"{name} precision {prec}: rel_error {rel} (2^{int(np.log2(rel))}), {early:.3f} of the pixels freeze before the end, "
          f"{np.mean(first == 0):.3f} never, {np.mean(first == 2):.3f} at the first chance")
    assert 0.25 <= early <= 0.75 and len(np.unique(first)) >= 4  # about half, and not all in one pass
    expect = shot.copy()
    for k in sorted(plain):
        expect[first == k] = plain[k][0][first == k]
    assert_images_equal(frame, expect, f"{name} adaptive: frozen pixels vs plain previews, the rest vs the one-shot frame")
    n_i = np.where(first != 0, first, 8)
    assert (counts == n_i).all() and st.primary_rays == int(n_i.sum())
    assert (frame != shot).any()  # the freezing is visible in the frame
