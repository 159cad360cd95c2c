"""Adaptive passes on the GPU (rayz_hip_progressive_set_adaptive / _adaptive_step / _run_adaptive, rayz_hip_adaptive_kat; DESIGN.md
§4.14): fold, freeze and compaction against the numpy restatement bit for bit, and whole renders against plain handles stepped
over the same boundaries — a frozen pixel IS the plain preview at the chunk it froze at, a pixel that never froze IS the one-shot
pixel."""
import numpy as np
import pytest
import torch

import adaptive_cases
import adaptive_ref
import denoise_guided_ref
import noise_ref
from helpers import assert_images_equal
from rayz_amd import capi, render, tracer

pytestmark = pytest.mark.gpu

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR, BVH = capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH
ALL = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b, what):  # bit for bit, any NaN equal to any NaN
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    ok = (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))
    assert ok.all(), f"{what}: {np.count_nonzero(~ok)} of {ok.size} differ, first at {np.argwhere(~ok)[:3].tolist()}"


def params(base, **kw):
    p = capi.RenderParams.from_buffer_copy(bytes(base))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def out_tensor(p):
    dt = torch.float64 if p.precision == F64 else torch.float32
    out = torch.full((render.shard_rows(p), p.width, 3), float("nan"), dtype=dt, device="cuda")
    torch.cuda.synchronize()
    return out


def scene(width=96, spp=256, prec=F32, trav=capi.TRAVERSAL_AUTO, max_bounces=12):
    t = tracer.randomBouncing(width, seed=7)  # 96x54: ~485 spheres, every material + checker + motion blur
    t.samples_per_px, t.max_bounces = spp, max_bounces
    t.set_gpu(render_seed=11, precision=prec, traversal=trav, tmin=1e-3 if prec == F32 else 1e-10)
    return t


def adaptive_render(ds, cam, p, rel_error, min_chunks, min_samples=32, stepwise=True):
    """An adaptive handle run to its end, one buffer through every pass.  Returns frame, frozen_at, counts (numpy), the summaries
    of the passes, and the handle's RenderStats."""
    pr = ds.progressive(cam, p, adaptive=True, min_chunks=min_chunks)
    try:
        out, sms = out_tensor(p), []
        if stepwise:
            while True:
                sm = pr.adaptive_step(rel_error=rel_error, min_samples=min_samples, out=out)
                sms.append(sm)
                if sm.active == 0 or pr.done:
                    break
        else:
            sms.append(pr.render_adaptive(rel_error=rel_error, min_samples_per_pass=min_samples, out=out))
        return {"frame": out.cpu().numpy(), "frozen_at": pr.frozen_at().cpu().numpy(), "counts": pr.sample_counts().cpu().numpy(),
                "summaries": sms, "stats": pr.stats(), "chunks_done": pr.chunks_done}
    finally:
        pr.close()


def plain_steps(ds, cam, p, min_samples=32, rel_error=0.0625, rgb=False):
    """A plain tracked handle over the same boundaries: {chunks_done: (preview, var, rel2[, var_rgb])} and the boundaries."""
    pr = ds.progressive(cam, p, track_noise=True)
    seen = {}
    try:
        while not pr.done:
            out = out_tensor(p)
            pr.step(min_samples, out.data_ptr())
            _, var, rel2 = pr.noise(rel_error=rel_error, var=True, rel2=True)
            entry = [out.cpu().numpy(), var.cpu().numpy(), rel2.cpu().numpy()]
            if rgb:
                v3 = pr.noise_rgb()
                pr.stats()
                entry.append(v3.cpu().numpy())
            seen[pr.chunks_done] = entry
        return seen
    finally:
        pr.close()


# ---- 1. the kernels against the restatement, bit for bit --------------------------------------------------------------------
SCHEDULES = {"6x16": ([16] * 6, [1, 2, 3, 4, 6]), "auto": ([256, 256, 128, 64, 32, 16, 16], [1, 2, 3, 4, 5, 7])}


def synthetic_sums(n, sizes, rng):
    """Chunk sums n_k · level_i · (1 + a_i · u): every pixel has its own level and its own noise amplitude a_i, log-uniform over
    0.01 .. 1 and independent of its index — so each pass freezes a different, non-contiguous subset (the calm ones first), the
    wildest never freeze, and the first pass (one chunk: no estimate) freezes nobody.  A NaN pixel and a black one ride along."""
    K = len(sizes)
    sz = np.asarray(sizes, dtype=np.float64).reshape(K, 1, 1)
    level = (1.0 + np.arange(n) / n).reshape(1, n, 1) * np.array([1.0, 0.5, 0.25]).reshape(1, 1, 3)
    amp = 10.0 ** rng.uniform(-2, 0, size=(1, n, 1))
    sums = level * sz * (1.0 + amp * rng.uniform(-1, 1, size=(K, n, 3)))
    if n > 3:
        sums[0, 3, 1] = np.nan
        sums[:, 2] = 0.0
    return sums


@pytest.mark.parametrize("prec", [F32, F64])
@pytest.mark.parametrize("sched", list(SCHEDULES), ids=list(SCHEDULES))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_kat_matches_the_restatement_bit_for_bit(gpu, n, sched, prec):
    sizes, ends = SCHEDULES[sched]
    sums = synthetic_sums(n, sizes, np.random.default_rng(100 * n + prec))
    prm = {"rel_error": 0.05, "mean_floor": 0.02, "min_chunks": 2}
    got = render.adaptive_kat(sums, sizes, ends, prec, **prm)
    want = adaptive_ref.run(sums, sizes, ends, f64=prec == F64, **prm)
    assert (got["frozen_at"] == want["frozen_at"]).all()
    same(got["acc"], want["acc"], "acc")
    same(got["Q"], want["Q"], "Q")
    same(got["frame"], want["frame"], "frame")
    assert len(got["lists"]) == len(ends) + 1
    for p, (g, w) in enumerate(zip(got["lists"], want["lists"])):
        assert g.tolist() == w.tolist(), f"active list {p}"
    for p in range(len(ends)):  # each list is the ordered compaction of the one before
        keep = [i for i in got["lists"][p].tolist() if not (0 < got["frozen_at"][i] <= ends[p])]
        assert got["lists"][p + 1].tolist() == keep
    if n >= 63:  # the passes differ: one that freezes nobody, then shrinking non-contiguous subsets, and some pixels are left
        left = [len(l) for l in got["lists"]]
        assert left[0] == left[1] == n and len(set(left)) >= 4 and left[-1] > 0, left
        gone = np.flatnonzero(got["frozen_at"] == ends[1])
        assert len(gone) >= 2 and (np.diff(gone) > 1).any()


@pytest.mark.parametrize("prec", [F32, F64])
def test_kat_everything_freezes_nothing_freezes_and_the_dealing_order(gpu, prec):
    sizes, ends = [16] * 6, [1, 2, 3, 4, 5, 6]
    calm = np.ones((6, 300, 3)) * 16.0
    got = render.adaptive_kat(calm, sizes, ends, prec, min_chunks=3)  # one pass freezes everything: the run ends there
    assert (got["frozen_at"] == 3).all() and [len(l) for l in got["lists"]] == [300, 300, 300, 0, 0, 0, 0]
    same(got["frame"], np.ones((300, 3)), "frame")
    rng = np.random.default_rng(5)
    wild = 16.0 * rng.uniform(0.0, 2.0, size=(6, 300, 3))
    got = render.adaptive_kat(wild, sizes, ends, prec, rel_error=1e-9, min_chunks=2)  # nothing ever freezes: the full fold
    want = adaptive_ref.run(wild, sizes, ends, f64=prec == F64, rel_error=1e-9, min_chunks=2)
    assert (got["frozen_at"] == 0).all() and all(l.tolist() == list(range(300)) for l in got["lists"])
    same(got["frame"], want["frame"], "frame")
    M, _ = noise_ref.fold(wild, sizes, prec == F64)
    same(got["acc"], M, "acc vs the plain fold")
    # a 24x20 shard: two tile rows of three 8x8 tiles, then four rows dealt as they come; and a width that is no multiple of 8
    for w, n in ((24, 480), (10, 300)):
        sums = synthetic_sums(n, sizes, rng)
        got = render.adaptive_kat(sums, sizes, ends, prec, min_chunks=2, width=w)
        want = adaptive_ref.run(sums, sizes, ends, f64=prec == F64, min_chunks=2, width=w)
        assert got["lists"][0].tolist() == adaptive_ref.deal_order(n, w).tolist()
        assert all(g.tolist() == x.tolist() for g, x in zip(got["lists"], want["lists"])) and (got["frozen_at"] == want["frozen_at"]).all()
        same(got["frame"], want["frame"], "frame")


@pytest.mark.parametrize("prec", [F32, F64])
def test_kat_gives_the_hand_worked_answers(gpu, prec):
    c = adaptive_cases
    got = render.adaptive_kat(c.SUMS, c.SIZES, c.PASS_ENDS, prec, **c.PARAMS)
    assert got["frozen_at"].tolist() == c.WANT_FROZEN_AT and [l.tolist() for l in got["lists"]] == c.WANT_LISTS
    same(got["frame"][:, 0], c.WANT_RED, "red")
    same(got["acc"][:, 0], c.WANT_ACC_RED, "acc")
    same(got["Q"][:, 0], c.WANT_Q_RED, "Q")


# ---- 2. frames against plain handles ------------------------------------------------------------------------------------------
REL_ERROR = 0.0625  # (moved from the run-until test's 0.25, at which every pixel of this frame freezes by 64 samples: see the frames test)


def check_against_plain(ad, plain, one_shot, p, min_chunks, what):
    tau2 = np.float32(REL_ERROR * REL_ERROR)  # (exact in f32, so rel2's single rounding to f32 cannot cross it: the f32 output decides as the f64 value did)
    assert float(tau2) == REL_ERROR * REL_ERROR
    bounds = sorted(plain)
    first = np.zeros(ad["frozen_at"].shape, dtype=np.int64)
    for k in reversed(bounds):
        if k >= min_chunks:
            first[plain[k][2] <= tau2] = k
    assert (ad["frozen_at"] == first).all(), f"{what}: frozen_at differs at {np.argwhere(ad['frozen_at'] != first)[:4].tolist()}"
    want = one_shot.copy()
    for k in bounds:
        want[first == k] = plain[k][0][first == k]
    assert_images_equal(ad["frame"], want, f"{what}: frozen pixels vs plain previews, the rest vs the one-shot frame")
    spp = p.samples_per_px
    n_of = np.array([0] + [min(p.chunk_spp * k, spp) for k in range(1, bounds[-1] + 1)])
    counts = np.where(first != 0, n_of[first], spp)
    assert (ad["counts"] == counts).all()
    last = ad["summaries"][-1]
    assert int(counts.sum()) == ad["stats"].primary_rays == last.samples_traced
    assert last.pixels == counts.size and last.active == np.count_nonzero(first == 0)
    return first


@pytest.mark.parametrize("prec", [F32, F64])
def test_frames_equal_plain_handles_pixel_by_pixel(gpu, prec):
    """randomBouncing at 96x54 (48 tiled rows plus 6 dealt by row), 256 spp in chunks of 16, passes of 32 samples, min_chunks 2.
    The test needs at least 10 % of the pixels to freeze before the end and at least 1 % never to freeze.  At rel_error 0.25 the
    plain handle's own estimate, evaluated at every boundary, freezes ALL 5,184 pixels by 64 samples (none is left), so rel_error
    was moved to 0.0625 (its square, 1/256, is exact in f32): there 3,969 pixels (76.6 %) freeze before the end and 1,009 (19.5 %)
    never freeze in f32, 3,968 and 1,005 in f64 (0.125: 99.6 % / 0.2 %; 0.03125: 37.2 % / 61.9 %).
    BVH and flat list give the same bits."""
    results = {}
    for trav in (BVH, LINEAR):
        t = scene(96, 256, prec, trav)
        p = params(t.params(), chunk_spp=16)
        cam = t.camera_desc()
        ds = gpu.DeviceScene(t.scene_desc())
        try:
            one_shot = out_tensor(p)
            ds.render_into(cam, p, one_shot.data_ptr())
            ds.sync()
            one_shot = one_shot.cpu().numpy()
            ad = adaptive_render(ds, cam, p, REL_ERROR, 2)
            if trav == BVH:
                plain = plain_steps(ds, cam, p)
                first = check_against_plain(ad, plain, one_shot, p, 2, "BVH")
                early, never = np.count_nonzero((first != 0) & (first < 16)), np.count_nonzero(first == 0)
                print(f"precision {prec}: {early} of {first.size} pixels freeze before the end, {never} never freeze")
                assert early >= 0.10 * first.size and never >= 0.01 * first.size, (early, never)
                whole = adaptive_render(ds, cam, p, REL_ERROR, 2, stepwise=False)  # run_adaptive: the same frame in one call
                assert_images_equal(whole["frame"], ad["frame"], "run_adaptive vs the steps")
                assert (whole["frozen_at"] == ad["frozen_at"]).all()
                assert whole["summaries"][-1].samples_traced == ad["summaries"][-1].samples_traced
            results[trav] = ad
        finally:
            ds.close()
    assert_images_equal(results[LINEAR]["frame"], results[BVH]["frame"], "flat list vs BVH")
    assert (results[LINEAR]["frozen_at"] == results[BVH]["frozen_at"]).all() and (results[LINEAR]["counts"] == results[BVH]["counts"]).all()


# ---- 3. nothing freezes / 4. everything freezes ----------------------------------------------------------------------------------
def test_nothing_freezes_gives_the_one_shot_frame(gpu):
    """rel_error 1e-9.  No positive rel_error keeps a pixel whose chunk sums agree EXACTLY from freezing (rel2 = 0: this frame has
    a few black pixels, 27 of 5,184 by the end), so the case is held twice: with min_chunks beyond the schedule nothing can freeze —
    every pass traces every pixel and the frame is the one-shot frame in every pixel; with min_chunks 2 the pixels that froze are
    exactly those whose estimate is exactly zero, and every other pixel is the one-shot pixel."""
    t = scene(96, 64)
    p = params(t.params(), chunk_spp=16)
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        want = out_tensor(p)
        ds.render_into(t.camera_desc(), p, want.data_ptr())
        ds.sync()
        want = want.cpu().numpy()
        ad = adaptive_render(ds, t.camera_desc(), p, 1e-9, 5, min_samples=0)
        pr = ds.progressive(t.camera_desc(), p, adaptive=True, min_chunks=2)
        out = out_tensor(p)
        sm = pr.render_adaptive(rel_error=1e-9, min_samples_per_pass=0, out=out)
        _, var, rel2 = pr.noise(rel_error=1e-9, var=True, rel2=True)
        frozen, var, rel2, frame = pr.frozen_at().cpu().numpy(), var.cpu().numpy(), rel2.cpu().numpy(), out.cpu().numpy()
        pr.close()
    finally:
        ds.close()
    assert [s.active for s in ad["summaries"]] == [96 * 54] * 4 and [s.chunks_done for s in ad["summaries"]] == [1, 2, 3, 4]
    assert (ad["frozen_at"] == 0).all() and (ad["counts"] == 64).all() and ad["stats"].primary_rays == 96 * 54 * 64
    assert_images_equal(ad["frame"], want, "an adaptive run in which nothing could freeze vs one-shot")
    assert sm.chunks_done == 4 and sm.active == np.count_nonzero(frozen == 0) > 0.99 * frozen.size
    assert (rel2[frozen != 0] == 0).all() and (var[frozen != 0] == 0).all() and (rel2[frozen == 0] > 0).all()
    assert_images_equal(frame[frozen == 0], want[frozen == 0], "the pixels that never froze vs one-shot")


@pytest.mark.parametrize("min_chunks", [2, 3])
def test_everything_freezes_with_no_bounces(gpu, min_chunks):
    t = scene(96, 128, max_bounces=0)
    p = params(t.params(), chunk_spp=16)
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        pr = ds.progressive(t.camera_desc(), p, adaptive=True, min_chunks=min_chunks)
        out = out_tensor(p)
        sms = [pr.adaptive_step(min_samples=0, out=out) for _ in range(min_chunks + 2)]
        other = out_tensor(p)
        late = pr.adaptive_step(min_samples=0, out=other)  # a finished run: traces nothing, writes the frame it is asked for
        done_early = not pr.done
        frozen, counts, frame, frame2 = pr.frozen_at().cpu().numpy(), pr.sample_counts().cpu().numpy(), out.cpu().numpy(), other.cpu().numpy()
        rays = pr.stats().primary_rays
        pr.close()
        pr = ds.progressive(t.camera_desc(), p, adaptive=True, min_chunks=min_chunks)
        whole = pr.render_adaptive(min_samples_per_pass=0)
        pr.close()
    finally:
        ds.close()
    want_active = [96 * 54] * (min_chunks - 1) + [0] * 3
    assert [s.active for s in sms] == want_active
    assert [s.passes for s in sms] == list(range(1, min_chunks)) + [min_chunks] * 3 and late.passes == min_chunks
    assert [s.chunks_done for s in sms][-3:] == [min_chunks] * 3 and done_early
    assert (frozen == min_chunks).all() and (counts == 16 * min_chunks).all() and rays == 96 * 54 * 16 * min_chunks
    assert (frame == 0).all() and (frame2 == 0).all()
    assert (whole.passes, whole.chunks_done, whole.active, whole.samples_traced) == (min_chunks, min_chunks, 0, rays)


# ---- 5. shards ----------------------------------------------------------------------------------------------------------------
def test_a_shard_gives_the_whole_frames_rows(gpu):
    t = scene(96, 128)
    p = params(t.params(), chunk_spp=16)
    ps = params(p, shard_index=1, shard_count=3, tile_rows=8)
    rows = render.shard_row_indices(p.height, 8, 1, 3)
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        whole = adaptive_render(ds, t.camera_desc(), p, REL_ERROR, 2)
        shard = adaptive_render(ds, t.camera_desc(), ps, REL_ERROR, 2)
    finally:
        ds.close()
    assert shard["frozen_at"].shape == (len(rows), 96) and 0 < np.count_nonzero(shard["frozen_at"]) < shard["frozen_at"].size
    assert (shard["frozen_at"] == whole["frozen_at"][rows]).all() and (shard["counts"] == whole["counts"][rows]).all()
    assert_images_equal(shard["frame"], whole["frame"][rows], "shard 1 of 3 vs the whole frame's rows")


# ---- 6. the noise entries on an adaptive handle -------------------------------------------------------------------------------
def test_noise_entries_use_every_pixels_own_chunk_count(gpu):
    """var, rel2 and var_rgb of an adaptive handle are, per pixel, the plain handle's at the boundary the pixel froze at (the end
    for one that never froze) — and, where N_i is a power of two (M = frame x N_i exactly), noise_ref.evaluate's with (K_i, N_i).
    The adaptive frame and its noise_rgb go through Denoiser.run_guided and equal the guided mirror on the same downloads."""
    t = scene(96, 256, F32, BVH)
    p = params(t.params(), chunk_spp=16)
    cam = t.camera_desc()
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        plain = plain_steps(ds, cam, p, rgb=True)
        pr = ds.progressive(cam, p, adaptive=True, min_chunks=2)
        frame = out_tensor(p)
        last = pr.render_adaptive(rel_error=REL_ERROR, min_samples_per_pass=32, out=frame)
        sm, var, rel2 = pr.noise(rel_error=REL_ERROR, var=True, rel2=True)
        v3 = pr.noise_rgb()
        pr.stats()
        frozen, Q = pr.frozen_at().cpu().numpy(), pr.noise_state().cpu().numpy()[..., :3]
        var, rel2, v3h, frame_h = var.cpu().numpy(), rel2.cpu().numpy(), v3.cpu().numpy(), frame.cpu().numpy()
        g = ds.gbuffer(cam, p)
        ds.query_sync()
        dn = render.Denoiser(p.width, p.height)
        out, vout = dn.run_guided(frame, v3, g, var_out=True)
        torch.cuda.synchronize()
        out_h, vout_h = out.cpu().numpy(), vout.cpu().numpy()
        host = [getattr(g, k).cpu().numpy() for k in ("index", "normal", "point", "albedo")]
        dn.close()
        pr.close()
    finally:
        ds.close()
    assert (sm.chunks_done, sm.samples_done) == (last.chunks_done, last.samples_done) == (16, 256)
    K = np.where(frozen != 0, frozen, 16)
    assert len(np.unique(K)) >= 4
    for k in np.unique(K):
        m = K == k
        same(var[m], plain[k][1][m], f"var at K = {k}")
        same(rel2[m], plain[k][2][m], f"rel2 at K = {k}")
        same(v3h[m], plain[k][3][m], f"var_rgb at K = {k}")
        if k in (2, 4, 8, 16):
            M = frame_h[m].astype(np.float64) * (16.0 * k)
            wv, wr, _ = noise_ref.evaluate(M, Q[m], int(k), 16 * int(k), REL_ERROR)
            same(var[m], wv.astype(np.float32), f"var vs the restatement at K = {k}")
            same(rel2[m], wr.astype(np.float32), f"rel2 vs the restatement at K = {k}")
    assert sm.unconverged == np.count_nonzero(frozen == 0)  # evaluated with the parameters it froze by
    want = denoise_guided_ref.denoise(frame_h, v3h, *host, **capi.DENOISE_GUIDED_DEFAULTS)
    same(out_h, want[0], "run_guided on an adaptive frame")
    same(vout_h, want[1], "run_guided on an adaptive frame (variance)")


# ---- 7. mode and ordering -----------------------------------------------------------------------------------------------------
def test_mode_refusals(gpu):
    t = scene(48, 64)
    p = params(t.params(), chunk_spp=16)
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        pr = ds.progressive(t.camera_desc(), p, track_noise=True)
        pr.step(0)
        with pytest.raises(capi.RayzHipError, match="before the first step"):
            pr.set_adaptive(2)
        with pytest.raises(capi.RayzHipError, match="not in adaptive mode"):
            pr.adaptive_step()
        with pytest.raises(capi.RayzHipError, match="not in adaptive mode"):
            pr.sample_counts()
        pr.close()
        with pytest.raises(capi.RayzHipError, match="min_chunks 1"):
            ds.progressive(t.camera_desc(), p, adaptive=True, min_chunks=1)
        pr = ds.progressive(t.camera_desc(), p, adaptive=True, min_chunks=2)
        with pytest.raises(capi.RayzHipError, match="adaptive mode"):
            pr.step(0)
        with pytest.raises(capi.RayzHipError, match="adaptive mode"):
            pr.render_until()
        assert pr.chunks_done == 0
        pr.adaptive_step()
        with pytest.raises(capi.RayzHipError, match="before the first step"):
            pr.set_adaptive(3)
        pf = ds.progressive(t.camera_desc(), params(p, precision=F64, tmin=1e-10), adaptive=True)
        with pytest.raises(capi.RayzHipError, match="precision"):
            capi.check(pf._lib, pf._lib.rayz_hip_progressive_adaptive_step(pf._h, None, 0, None, None, None), "step")
        pf.close()
        pr.close()  # destroyed mid-run
    finally:
        ds.close()


def test_streams_buffers_and_other_renders_between_steps(gpu):
    """Passes on alternating streams, each into a fresh buffer (so each writes the whole frame), with a one-shot render and a
    camera query on the same scene between them: the end is the frame of the undisturbed run."""
    t = scene(96, 128)
    p = params(t.params(), chunk_spp=16)
    cam = t.camera_desc()
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        calm = adaptive_render(ds, cam, p, REL_ERROR, 2)
        side = torch.cuda.Stream()
        pr = ds.progressive(cam, p, adaptive=True, min_chunks=2)
        other, i, sm = out_tensor(params(p, samples_per_px=16)), 0, None
        while sm is None or (sm.active and not pr.done):
            out = out_tensor(p)
            sm = pr.adaptive_step(rel_error=REL_ERROR, min_samples=32, out=out, stream=side.cuda_stream if i % 2 else 0)
            ds.render_into(cam, params(p, samples_per_px=16), other.data_ptr())
            ds.sync()
            ds.gbuffer(cam, p, outputs=("index",))
            ds.query_sync()
            i += 1
        frame, frozen = out.cpu().numpy(), pr.frozen_at(stream=side.cuda_stream).cpu().numpy()
        pr.close()
    finally:
        ds.close()
    assert i >= 3
    assert_images_equal(frame, calm["frame"], "disturbed vs undisturbed adaptive run")
    assert (frozen == calm["frozen_at"]).all()


def test_preview_after_a_pass_without_a_buffer_is_whole(gpu):
    """The preview rule's other branch: buffer A, no buffer, buffer A again (a preview refreshed every second pass).  The pass
    without a buffer wrote nothing, so the next pass into A writes every pixel: the pixels that froze in between hold their final
    value, not the one A kept from two passes before.  Held after every pass into A against the undisturbed run's buffer (one
    tensor through every pass) after the same pass."""
    t = scene(96, 128)
    p = params(t.params(), chunk_spp=16)
    cam = t.camera_desc()
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        calm, gappy, frozen = [], [], None
        for every in (1, 2):
            pr = ds.progressive(cam, p, adaptive=True, min_chunks=2)
            out, i = out_tensor(p), 0
            while True:
                sm = pr.adaptive_step(rel_error=REL_ERROR, min_samples=32, out=out if i % every == 0 else None)
                (calm if every == 1 else gappy).append(out.cpu().numpy() if i % every == 0 else None)
                i += 1
                if sm.active == 0 or pr.done:
                    break
            frozen = pr.frozen_at().cpu().numpy()
            pr.close()
    finally:
        ds.close()
    assert len(calm) == len(gappy) == 4 and gappy[1] is None and gappy[3] is None
    in_the_gap = frozen == 4  # (pass 2, the one without a buffer, ends at chunk 4)
    assert in_the_gap.any() and (calm[0][in_the_gap] != calm[2][in_the_gap]).any()  # the stale value would be visible
    assert_images_equal(gappy[0], calm[0], "pass 1 into A")
    assert_images_equal(gappy[2], calm[2], "pass 3 into A, after a pass without a buffer")
