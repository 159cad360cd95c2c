"""Progressive rendering (rayz_hip_progressive_*, `DeviceScene.progressive`) on the GPU.

A progressive render traces the frame in passes of whole chunks of its chunk schedule and folds each pass's chunk sums into
an accumulator in chunk order: once every chunk is covered it has made resolve_kernel's additions in resolve_kernel's order,
so its frame is the one-shot frame bit for bit, whatever the passes were; in between, the preview is the mean of a prefix of
exactly the samples the final frame averages."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from helpers import assert_images_equal
from rayz_amd import capi, render, tracer

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR, BVH = capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH
ALL = 0xFFFFFFFF


def params(base, **kw):
    p = capi.RenderParams.from_buffer_copy(bytes(base))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def schedule(p):
    buf = (C.c_uint32 * 256)()
    n = capi.load().rayz_hip_chunk_schedule(C.byref(p), buf, 256)
    assert 0 < n < 256
    return list(buf[: n + 1])


def out_tensor(p):
    """A frame buffer pre-filled with NaN (every value must be written), synchronised before the library's own stream uses it."""
    dt = torch.float64 if p.precision == F64 else torch.float32
    out = torch.full((render.shard_rows(p), p.width, 3), float("nan"), dtype=dt, device="cuda")
    torch.cuda.synchronize()
    return out


def one_shot(ds, cam, p):
    out = out_tensor(p)
    ds.render_into(cam, p, out.data_ptr())
    st = ds.sync()
    return out.cpu().numpy(), st


def min_samples_for(pr_sched, c0, m):
    """min_samples that makes a step from chunk c0 cover exactly m chunks (the fewest whole chunks adding that many)."""
    return pr_sched[c0 + m - 1] - pr_sched[c0] + 1


def progressive(ds, cam, p, chunk_steps=None, mins=None, previews=False):
    """Steps a progressive render to the end: `chunk_steps` = chunks per step (cycled), or `mins` = min_samples per step.
    Returns (final frame, stats, {chunks_done: preview} if previews)."""
    sched = schedule(p)
    pr = ds.progressive(cam, p)
    seen = {}
    try:
        assert pr.n_chunks == len(sched) - 1 and pr.samples_done == 0 and not pr.done
        i = 0
        while not pr.done:
            c0 = pr.chunks_done
            if mins is not None:
                m = mins[i % len(mins)]
            else:
                m = min_samples_for(sched, c0, min(chunk_steps[i % len(chunk_steps)], len(sched) - 1 - c0))
            out = out_tensor(p)
            pr.step(m, out.data_ptr())
            assert pr.samples_done == sched[pr.chunks_done] and pr.chunks_done > c0
            if previews:
                pr.stats()  # (waits for the pass)
                seen[pr.chunks_done] = out.cpu().numpy()
            i += 1
        st = pr.stats()
        final = out.cpu().numpy()
        return final, st, seen
    finally:
        pr.close()


def scene_96(seed=7):
    t = tracer.randomBouncing(96, seed=seed)  # 96x54, ~485 spheres, every material + checker + motion blur
    t.samples_per_px, t.max_bounces = 48, 12
    t.set_gpu(render_seed=11)
    return t


# ---- 1. the end is the one-shot frame --------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [F32, F64])
@pytest.mark.parametrize("trav", [LINEAR, BVH])
@pytest.mark.parametrize("sched", ["uniform", "odd"])
def test_final_frame_is_the_one_shot_frame_and_the_oracle(gpu, oracle, prec, trav, sched):
    t = scene_96()
    scene, cam = t.scene_desc(), t.camera_desc()
    p = params(t.params(), precision=prec, traversal=trav, tmin=1e-3 if prec == F32 else 1e-10)
    if sched == "odd":  # an explicit chunk size that does not divide spp: a short last chunk
        p = params(p, samples_per_px=50, chunk_spp=7)
        assert schedule(p)[-2:] == [49, 50]
    ds = gpu.DeviceScene(scene)
    try:
        want, st1 = one_shot(ds, cam, p)
        got, st, _ = progressive(ds, cam, p, chunk_steps=[1])
    finally:
        ds.close()
    assert_images_equal(got, want, f"progressive vs one-shot ({sched}, prec {prec}, traversal {trav})")
    ref, _ = oracle.render_b(scene, cam, p)
    assert_images_equal(got, ref, "progressive vs oracle mode B")
    assert st.primary_rays == 96 * 54 * p.samples_per_px and st.segments == st1.segments


@pytest.mark.parametrize("prec,trav", [(F32, LINEAR), (F32, BVH), (F64, LINEAR), (F64, BVH)])
def test_automatic_non_uniform_schedule(gpu, prec, trav):
    """1024x576 at 64 spp: the automatic schedule is 32, 16, 16 (not uniform), so windows after the first read the tail of
    the table — the trace kernel's uniform-prefix shortcut must not be applied to them."""
    t = tracer.randomBouncing(1024, -2, 2, seed=3)
    t.samples_per_px, t.max_bounces = 64, 8
    t.set_gpu(render_seed=5, precision=prec, traversal=trav, tmin=1e-3 if prec == F32 else 1e-10)
    p = t.params()
    assert p.width * p.height >= 1 << 19 and schedule(p) == [0, 32, 48, 64]
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        want, st1 = one_shot(ds, t.camera_desc(), p)
        got, st, _ = progressive(ds, t.camera_desc(), p, chunk_steps=[1])
        assert_images_equal(got, want, "one chunk per pass")
        got2, _, _ = progressive(ds, t.camera_desc(), p, chunk_steps=[2, 1])  # the first pass covers 32 + 16
        assert_images_equal(got2, want, "two chunks, then one")
    finally:
        ds.close()
    assert st.segments == st1.segments and st.primary_rays == st1.primary_rays


# ---- 2. any partition, and equal previews at equal chunk counts -------------------------------------------------------------
@pytest.mark.parametrize("prec,trav", [(F32, BVH), (F64, LINEAR)])
def test_any_partition_gives_the_same_bits(gpu, prec, trav):
    t = scene_96()
    t.samples_per_px = 160  # ten chunks of 16
    p = params(t.params(), precision=prec, traversal=trav)
    cam = t.camera_desc()
    n = len(schedule(p)) - 1
    assert n == 10
    rng = np.random.default_rng(1)
    parts = []
    left = n
    while left:
        k = int(rng.integers(1, min(left, 4) + 1))
        parts.append(k)
        left -= k
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        want, _ = one_shot(ds, cam, p)
        runs = {"ones": progressive(ds, cam, p, chunk_steps=[1], previews=True),
                "twos": progressive(ds, cam, p, chunk_steps=[2], previews=True),
                f"random {parts}": progressive(ds, cam, p, chunk_steps=parts, previews=True),
                "all": progressive(ds, cam, p, mins=[ALL], previews=True)}
    finally:
        ds.close()
    assert set(runs["all"][2]) == {n}
    for name, (final, _, seen) in runs.items():
        assert_images_equal(final, want, f"{name}: final frame")
        for c, img in seen.items():
            assert_images_equal(img, runs["ones"][2][c], f"{name}: preview after {c} chunks vs one chunk per pass")


# ---- 3. a preview is a prefix mean -----------------------------------------------------------------------------------------
def test_preview_is_a_prefix_mean(gpu):
    t = scene_96()
    t.samples_per_px = 256
    p = t.params()
    sched = schedule(p)
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        final, _, seen = progressive(ds, t.camera_desc(), p, chunk_steps=[1], previews=True)
        # samples_done follows the schedule (checked at every step by progressive()); min_samples = 40 takes 3 chunks of 16
        pr = ds.progressive(t.camera_desc(), p)
        pr.step(40)
        assert pr.chunks_done == 3 and pr.samples_done == 48
        pr.step(0)
        assert pr.chunks_done == 4 and pr.samples_done == sched[4]
        pr.step(ALL)
        assert pr.done and pr.samples_done == 256
        with pytest.raises(capi.RayzHipError, match="status -5"):
            pr.step(0)
        pr.close()
    finally:
        ds.close()
    n = len(sched) - 1
    first, half = seen[1], seen[n // 2]
    assert not np.array_equal(first, final) and not np.array_equal(half, final)
    # the half-way preview averages the first half of every pixel's samples, the frame all of them: their difference is
    # noise (the two halves are independent), centred on 0 with no structure
    d = (half.astype(np.float64) - final).ravel()
    q1, q3 = np.percentile(d, [25, 75])
    sigma = max((q3 - q1) / 1.349, d.std() * 1e-3)
    print(f"half-way preview - frame: median {np.median(d):+.3e}, robust sigma {sigma:.3e}")
    assert abs(np.median(d)) < 0.05 * sigma
    assert abs(np.corrcoef(d, final.ravel())[0, 1]) < 0.2
    assert np.all(np.isfinite(half)) and np.all(half >= 0)


# ---- 4. shards ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("idx,count", [(1, 3), (0, 2)])
def test_shards(gpu, idx, count):
    t = scene_96()
    p = params(t.params(), shard_index=idx, shard_count=count, traversal=BVH)
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        want, st1 = one_shot(ds, t.camera_desc(), p)
        got, st, _ = progressive(ds, t.camera_desc(), p, chunk_steps=[1, 2])
    finally:
        ds.close()
    assert got.shape == (render.shard_rows(p), 96, 3)
    assert_images_equal(got, want, f"shard {idx} of {count}")
    assert st.primary_rays == render.shard_rows(p) * 96 * p.samples_per_px and st.segments == st1.segments


# ---- 5. other renders on the scene between steps ---------------------------------------------------------------------------
def test_other_renders_between_steps_change_nothing(gpu, oracle):
    t = scene_96()
    t.samples_per_px = 96  # six chunks of 16
    p = params(t.params(), traversal=BVH)
    cam = t.camera_desc()
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        want, _ = one_shot(ds, cam, p)
        pr = ds.progressive(cam, p)
        pr.step(40)
        assert pr.chunks_done == 3
        # a different spp and chunk schedule (the scene's cached table changes), on a larger frame (the workspace grows),
        # in the other precision and the flat list
        big = tracer.randomBouncing(160, seed=7)
        one_shot(ds, big.camera_desc(), params(p, width=160, height=90, samples_per_px=40, chunk_spp=5, traversal=LINEAR))
        one_shot(ds, cam, params(p, precision=F64, tmin=1e-10, samples_per_px=20, chunk_spp=3))
        out = out_tensor(p)
        pr.step(ALL, out.data_ptr())
        st = pr.stats()
        got = out.cpu().numpy()
        pr.close()
    finally:
        ds.close()
    assert_images_equal(got, want, "finished after other renders on the scene")
    ref, ost = oracle.render_b(t.scene_desc(), cam, p)
    assert_images_equal(got, ref, "vs oracle")
    assert st.segments == ost.segments


# ---- 6. edges --------------------------------------------------------------------------------------------------------------
def test_edges(gpu):
    t = scene_96()
    cam = t.camera_desc()
    ds = gpu.DeviceScene(t.scene_desc())
    lib = capi.load()
    try:
        # max_bounces = 0: black, as the one-shot render
        p0 = params(t.params(), max_bounces=0)
        got, st, _ = progressive(ds, cam, p0, chunk_steps=[1])
        assert (got == 0).all() and st.primary_rays == 96 * 54 * p0.samples_per_px and st.segments == 0
        # spp = 1: one step finishes it
        p1 = params(t.params(), samples_per_px=1)
        pr = ds.progressive(cam, p1)
        assert pr.n_chunks == 1
        pr.step(0)
        assert pr.done and pr.samples_done == 1
        # stepping a finished render is RAYZ_ERR_STATE
        assert lib.rayz_hip_progressive_step(pr._h, 0, None, None) == capi.ERR_STATE
        pr.close()
        # the entry of the other precision is RAYZ_ERR_BAD_ARG, and takes no step
        pr = ds.progressive(cam, t.params())
        assert lib.rayz_hip_progressive_step_f64(pr._h, 0, None, None) == capi.ERR_BAD_ARG
        assert b"precision" in lib.rayz_hip_last_error() and pr.chunks_done == 0
        pr.close()
        pr = ds.progressive(cam, params(t.params(), precision=F64, tmin=1e-10))
        assert lib.rayz_hip_progressive_step(pr._h, 0, None, None) == capi.ERR_BAD_ARG
        pr.close()
        # summed counters: primary rays = shard pixels x spp, segments = the one-shot render's; no preview pointer needed
        p = params(t.params(), traversal=LINEAR)
        _, st1 = one_shot(ds, cam, p)
        pr = ds.progressive(cam, p)
        while not pr.done:
            pr.step(0)
        st = pr.stats()
        pr.close()
        assert st.primary_rays == 96 * 54 * p.samples_per_px and st.segments == st1.segments
        assert st.sphere_tests == st1.sphere_tests and st.node_tests == 0 and st.kernel_ms > 0
    finally:
        ds.close()


# ---- 7. the CLI ------------------------------------------------------------------------------------------------------------
def test_cli_progress_line_and_same_image(gpu, tmp_path):
    exe = os.path.join(ROOT, "rayz_amd", "host", "rayz")
    env = dict(os.environ, RAYZ_SEED="7", RAYZ_SPP="3", RAYZ_BOUNCES="6")
    a, b = tmp_path / "a.ppm", tmp_path / "b.ppm"

    def run(out, **extra):  # stderr as bytes: text mode would turn the progress line's \r into \n
        r = subprocess.run([exe, "96", str(out)], capture_output=True, env=dict(env, **extra), timeout=600)
        err = r.stderr.decode()
        assert r.returncode == 0, err
        assert "Finished render (" in err and "rps and" in err
        return err.split("Finished render (")[0]

    assert "Progress" not in run(a)
    head = run(b, RAYZ_PROGRESS="1")
    assert head == "\rProgress: 100.00%\n", repr(head)  # 3 spp: one chunk, one pass
    assert a.read_bytes() == b.read_bytes()
    # 64 spp: passes of ~1/100 of the frame, rounded up to whole chunks of 16 -> one update per chunk
    head = run(b, RAYZ_PROGRESS="1", RAYZ_SPP="64")
    assert head == "\rProgress: 25.00%\rProgress: 50.00%\rProgress: 75.00%\rProgress: 100.00%\n", repr(head)
    run(a, RAYZ_SPP="64")
    assert a.read_bytes() == b.read_bytes()
