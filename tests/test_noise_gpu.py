"""The noise estimate of progressive rendering on the GPU (rayz_hip_progressive_track_noise / _noise / _run_until,
rayz_hip_noise_kat): the kernels against the numpy restatement bit for bit, and the properties the estimate
promises — tracking changes no image, the state does not depend on the partition into passes or on the shard layout, the
estimate is calibrated, and render-until-converged stops at a pass boundary on a prefix mean."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import noise_ref
from helpers import assert_images_equal
from noise_cases import CASES, CLAMP_CASE
from rayz_amd import capi, render, tracer

pytestmark = pytest.mark.gpu

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR, BVH = capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH
ALL = 0xFFFFFFFF


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


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


def scene(width=96, spp=256, seed=7, render_seed=11, **kw):
    t = tracer.randomBouncing(width, seed=seed)  # 96x54: ~485 spheres, every material + checker + motion blur
    t.samples_per_px, t.max_bounces = spp, 12
    t.set_gpu(render_seed=render_seed, **kw)
    return t


def run(ds, cam, p, mins, tracked=True, previews=False):
    """Steps a handle to the end with min_samples `mins` (the last entry repeats).  Returns a dict: final frame, Q, var, rel2
    (numpy; None untracked), summary, {chunks_done: preview}."""
    pr = ds.progressive(cam, p, track_noise=tracked)
    seen, i = {}, 0
    try:
        while not pr.done:
            out = out_tensor(p)
            pr.step(mins[min(i, len(mins) - 1)], out.data_ptr())
            if previews:
                pr.stats()
                seen[pr.chunks_done] = out.cpu().numpy()
            i += 1
        pr.stats()
        r = {"frame": out.cpu().numpy(), "previews": seen, "Q": None}
        if tracked:
            sm, var, rel2 = pr.noise(var=True, rel2=True)
            r.update(summary=sm, var=var.cpu().numpy(), rel2=rel2.cpu().numpy(), Q=pr.noise_state().cpu().numpy())
        return r
    finally:
        pr.close()


# ---- 1. the kernels against the restatement, bit for bit --------------------------------------------------------------------
def check_kat(sums, sizes, prec, **prm):
    q, var, rel2, sm = render.noise_kat(sums, sizes, prec, **prm)
    wq, wvar, wrel2, wsm = noise_ref.estimate(sums, sizes, prec == F64, **{**{"rel_error": noise_ref.DEFAULT_REL_ERROR,
                                                                                "mean_floor": noise_ref.DEFAULT_MEAN_FLOOR}, **prm})
    def same(a, b, what):  # bit for bit, except that any NaN equals any NaN (its payload and sign are not part of the contract)
        a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
        ok = (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))
        assert ok.all(), f"{what}: {np.count_nonzero(~ok)} of {ok.size} differ, first at {np.argwhere(~ok)[:3].tolist()}"
    same(q, wq, "Q")
    same(var, wvar, "var")
    same(rel2, wrel2, "rel2")
    assert (sm.pixels, sm.unconverged, sm.samples_done, sm.chunks_done) == (wsm["pixels"], wsm["unconverged"], wsm["samples_done"],
                                                                             wsm["chunks_done"])
    same([sm.max_rel2], [wsm["max_rel2"]], "max_rel2")
    assert sm.mean_var == pytest.approx(wsm["mean_var"], rel=1e-12, abs=0.0)
    return sm


SIZES = {"K1": [16], "K2": [16] * 2, "K3": [16] * 3, "K18": [16] * 18, "4+2": [4, 2], "auto": [256, 256, 128, 64, 32, 16, 16]}


@pytest.mark.parametrize("prec", [F32, F64])
@pytest.mark.parametrize("sizes", list(SIZES), ids=list(SIZES))
def test_kat_matches_the_restatement_bit_for_bit(gpu, sizes, prec):
    """1,296 pixels = five blocks of 256 and a 16-pixel tail; chunk sums over 12 decades of magnitude, some pixels with little
    spread between their chunks (D nearly cancels), some all zero, some dark (below the floor)."""
    sz = SIZES[sizes]
    n, K = 1296, len(sz)
    rng = np.random.default_rng(1000 * K + prec)
    mean = 10.0 ** rng.uniform(-6, 6, size=(1, n, 3))
    spread = 10.0 ** rng.uniform(-8, 0, size=(1, n, 1))
    sums = mean * (1.0 + spread * rng.standard_normal((K, n, 3))) * np.asarray(sz, dtype=np.float64).reshape(K, 1, 1)
    sums[:, 5] = 0.0
    sums[:, 1290] = sums[0, 1290]  # equal chunk sums in the tail block
    sm = check_kat(sums, sz, prec)
    assert sm.pixels == n
    check_kat(sums, sz, prec, rel_error=0.5, mean_floor=10.0)


@pytest.mark.parametrize("prec", [F32, F64])
def test_kat_closed_forms(gpu, prec):
    for name, sums, sizes, want in CASES + ([CLAMP_CASE] if prec == F32 else []):
        q, var, rel2, sm = render.noise_kat(sums, sizes, prec)
        for got, w in ((var[0], want["var"]), (rel2[0], want["rel2"]), (sm.max_rel2, want["rel2"])):
            assert got == w or (math.isnan(got) and math.isnan(w)), (name, got, w)
        if "q" in want:
            assert all(g == w or (math.isnan(g) and math.isnan(w)) for g, w in zip(q[0], want["q"])), (name, q, want["q"])
        assert sm.unconverged == want["unconverged"], name
        check_kat(sums, sizes, prec)
    # a NaN in one pixel of many surfaces in max_rel2 and counts once
    sums = np.ones((2, 700, 3))
    sums[1, 699, 2] = math.nan
    _, _, _, sm = render.noise_kat(sums, [1, 1], prec)
    assert math.isnan(sm.max_rel2) and sm.unconverged == 1 and sm.mean_var == 0.0


# ---- 2. tracking changes no image ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec,trav", [(F32, LINEAR), (F32, BVH), (F64, LINEAR), (F64, BVH)])
def test_tracking_changes_no_image(gpu, prec, trav):
    t = scene(48, 64, precision=prec, traversal=trav, tmin=1e-3 if prec == F32 else 1e-10)
    p = params(t.params(), chunk_spp=16)
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        want = out_tensor(p)
        ds.render_into(t.camera_desc(), p, want.data_ptr())
        ds.sync()
        a = run(ds, t.camera_desc(), p, [0], tracked=True, previews=True)
        b = run(ds, t.camera_desc(), p, [0], tracked=False, previews=True)
    finally:
        ds.close()
    assert sorted(a["previews"]) == sorted(b["previews"]) == [1, 2, 3, 4]
    for k in a["previews"]:
        assert_images_equal(a["previews"][k], b["previews"][k], f"preview after {k} chunks, tracked vs untracked")
    assert_images_equal(a["frame"], want.cpu().numpy(), "tracked final frame vs one-shot")
    assert_images_equal(b["frame"], want.cpu().numpy(), "untracked final frame vs one-shot")


# ---- 3. the state does not depend on the partition into passes ---------------------------------------------------------------
@pytest.mark.parametrize("prec", [F32, F64])
def test_partition_independence_and_the_first_chunk(gpu, prec):
    t = scene(96, 256, precision=prec, tmin=1e-3 if prec == F32 else 1e-10)
    p = params(t.params(), chunk_spp=16)
    cam = t.camera_desc()
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        one = run(ds, cam, p, [0])
        mixed = run(ds, cam, p, [17, 0, ALL])  # 2 chunks, 1 chunk, the rest
        whole = run(ds, cam, p, [ALL])
        pr = ds.progressive(cam, p, track_noise=True)  # the first step alone: Q = (S0 · S0) / n0, S0 = preview x 16 (exact)
        try:
            out = out_tensor(p)
            pr.step(0, out.data_ptr())
            q0 = pr.noise_state().cpu().numpy()
            sm0, var0, _ = pr.noise(var=True)
            S0 = out.cpu().numpy().astype(np.float64) * 16.0
            assert (sm0.chunks_done, sm0.samples_done, sm0.unconverged) == (1, 16, 96 * 54) and math.isinf(sm0.max_rel2)
            assert torch.isinf(var0).all()
        finally:
            pr.close()
    finally:
        ds.close()
    assert (bits(q0[..., :3]) == bits((S0 * S0) / 16.0)).all() and (q0[..., 3] == 0).all()
    for other, what in ((mixed, "[2, 1, rest]"), (whole, "one pass")):
        assert_images_equal(other["frame"], one["frame"], what)
        assert (bits(other["Q"]) == bits(one["Q"])).all(), what
        assert (bits32(other["var"]) == bits32(one["var"])).all() and (bits32(other["rel2"]) == bits32(one["rel2"])).all(), what
        assert other["summary"].unconverged == one["summary"].unconverged and other["summary"].max_rel2 == one["summary"].max_rel2
        assert other["summary"].mean_var == one["summary"].mean_var
    # the f32 outputs are the contract's f64 values rounded once: the restatement on the handle's own state (M = frame x 256, exact)
    M = one["frame"].astype(np.float64).reshape(-1, 3) * 256.0
    var, rel2, sm = noise_ref.evaluate(M, one["Q"].reshape(-1, 4)[:, :3], 16, 256)
    with np.errstate(over="ignore"):
        assert (bits32(one["var"].reshape(-1)) == bits32(var.astype(np.float32))).all()
        assert (bits32(one["rel2"].reshape(-1)) == bits32(rel2.astype(np.float32))).all()
    got = one["summary"]
    assert (got.pixels, got.unconverged, got.chunks_done, got.samples_done) == (96 * 54, sm["unconverged"], 16, 256)
    assert got.max_rel2 == sm["max_rel2"] and got.mean_var == pytest.approx(sm["mean_var"], rel=1e-12)
    assert 0 < got.unconverged < 96 * 54  # (a real image: some pixels done at 256 spp and 5 %, some not)


# ---- 4. shards ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("index,count", [(1, 3), (0, 2)])
def test_a_shard_estimates_the_whole_frames_rows(gpu, index, count):
    t = scene(96, 64)
    p = params(t.params(), chunk_spp=16)
    ps = params(p, shard_index=index, shard_count=count, tile_rows=8)
    rows = render.shard_row_indices(p.height, 8, index, count)
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        whole = run(ds, t.camera_desc(), p, [ALL])
        shard = run(ds, t.camera_desc(), ps, [0])
    finally:
        ds.close()
    assert shard["var"].shape == (len(rows), 96)
    assert (bits32(shard["var"]) == bits32(whole["var"][rows])).all() and (bits(shard["Q"]) == bits(whole["Q"][rows])).all()
    assert shard["summary"].pixels == len(rows) * 96


# ---- 5. calibration on the device ---------------------------------------------------------------------------------------------
def test_the_estimate_is_calibrated_on_the_device(gpu):
    """256 samples (K = 16) against an independent 4096-sample render of the same frame: the robust sigma of
    z = (mean - ref) / sqrt(var + var_ref) per channel must fall in the band measured on the CPU oracle (noise_ref.Z_SIGMA_BAND)."""
    t = scene(96, 256)
    p = params(t.params(), chunk_spp=16)
    pref = params(p, samples_per_px=4096, seed=p.seed + 12345)
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        a = run(ds, t.camera_desc(), p, [ALL])
        r = run(ds, t.camera_desc(), pref, [ALL])
    finally:
        ds.close()
    (K, N), (Kr, Nr) = ((x["summary"].chunks_done, x["summary"].samples_done) for x in (a, r))
    assert (N, Nr) == (256, 4096) and K >= 2 and Kr >= 2  # (powers of two: frame x N is the accumulator, exactly)
    z = noise_ref.z_sigma_from_moments(a["frame"].astype(np.float64).reshape(-1, 3) * N, a["Q"].reshape(-1, 4)[:, :3], K, N,
                                       r["frame"].astype(np.float64).reshape(-1, 3) * Nr, r["Q"].reshape(-1, 4)[:, :3], Kr, Nr)
    print(f"device z sigma: {z:.4f} (band {noise_ref.Z_SIGMA_BAND[0]:.4f} .. {noise_ref.Z_SIGMA_BAND[1]:.4f})")
    assert noise_ref.Z_SIGMA_BAND[0] <= z <= noise_ref.Z_SIGMA_BAND[1], z


# ---- 6. render until converged ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prec", [F32, F64])
def test_run_until_stops_at_a_pass_boundary_on_a_prefix_mean(gpu, prec):
    t = scene(96, 256, precision=prec, tmin=1e-3 if prec == F32 else 1e-10)
    p = params(t.params(), chunk_spp=16)
    cam = t.camera_desc()
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        pr = ds.progressive(cam, p, track_noise=True)
        try:
            out = out_tensor(p)
            sm = pr.render_until(rel_error=0.25, max_unconverged_fraction=0.05, min_samples_per_pass=32, out=out)
            assert sm.samples_done == pr.samples_done and sm.chunks_done == pr.chunks_done and not pr.done
            assert 32 < sm.samples_done < 256 and sm.samples_done % 32 == 0 and sm.unconverged <= 0.05 * sm.pixels
            early = out.cpu().numpy()
        finally:
            pr.close()
        plain = ds.progressive(cam, p)  # a plain handle stepped to the same chunk
        try:
            want = out_tensor(p)
            plain.step(sm.samples_done, want.data_ptr())
            assert plain.chunks_done == sm.chunks_done
            plain.stats()
            assert_images_equal(early, want.cpu().numpy(), f"run_until's frame at {sm.samples_done} samples vs the prefix mean")
        finally:
            plain.close()
        one = out_tensor(p)
        ds.render_into(cam, p, one.data_ptr())
        ds.sync()
        pr = ds.progressive(cam, p, track_noise=True)
        try:
            out = out_tensor(p)
            sm = pr.render_until(rel_error=1e-9, min_samples_per_pass=100, out=out)
            assert pr.done and (sm.samples_done, sm.chunks_done) == (256, 16) and sm.unconverged > 0
            assert_images_equal(out.cpu().numpy(), one.cpu().numpy(), "run_until to the end vs one-shot")
            with pytest.raises(capi.RayzHipError, match="finished"):
                pr.render_until()
        finally:
            pr.close()
    finally:
        ds.close()


def test_run_until_on_a_black_frame_converges_at_two_chunks(gpu):
    t = scene(96, 256)
    p = params(t.params(), chunk_spp=16, max_bounces=0)
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        pr = ds.progressive(t.camera_desc(), p, track_noise=True)
        try:
            out = out_tensor(p)
            sm = pr.render_until(out=out)
            assert (sm.chunks_done, sm.samples_done, sm.unconverged, sm.max_rel2, sm.mean_var) == (2, 32, 0, 0.0, 0.0)
            assert (out == 0).all()
        finally:
            pr.close()
    finally:
        ds.close()


# ---- 7. edges -----------------------------------------------------------------------------------------------------------------
def test_call_order_and_bad_parameters(gpu):
    lib = capi.load()
    t = scene(48, 64)
    p = params(t.params(), chunk_spp=16)
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        pr = ds.progressive(t.camera_desc(), p)
        try:
            sm = capi.NoiseSummary()
            assert lib.rayz_hip_progressive_noise(pr._h, None, None, None, C.byref(sm), None) == capi.ERR_STATE
            assert b"track" in lib.rayz_hip_last_error()
            assert lib.rayz_hip_progressive_run_until(pr._h, None, 0.0, 0, None, None, None) == capi.ERR_STATE
            assert lib.rayz_hip_progressive_track_noise(pr._h) == capi.OK
            assert lib.rayz_hip_progressive_track_noise(pr._h) == capi.OK  # again, before the first step: nothing
            for bad in (dict(rel_error=0.0), dict(rel_error=-1.0), dict(rel_error=math.nan), dict(mean_floor=0.0),
                        dict(mean_floor=math.nan), dict(rel_error=1e-200)):
                prm = capi.NoiseParams(**{**capi.NOISE_DEFAULTS, **bad})
                assert lib.rayz_hip_progressive_noise(pr._h, C.byref(prm), None, None, C.byref(sm), None) == capi.ERR_BAD_ARG, bad
                assert list(bad)[0].encode() in lib.rayz_hip_last_error()
                assert lib.rayz_hip_progressive_run_until(pr._h, C.byref(prm), 0.0, 0, None, None, None) == capi.ERR_BAD_ARG
            for frac in (-0.1, 1.5, math.nan):
                assert lib.rayz_hip_progressive_run_until(pr._h, None, frac, 0, None, None, None) == capi.ERR_BAD_ARG
            assert pr.chunks_done == 0  # (nothing above rendered)
            sm, _, _ = pr.noise()  # before the first step: no estimate
            assert (sm.chunks_done, sm.samples_done, sm.unconverged) == (0, 0, sm.pixels) and math.isinf(sm.max_rel2)
        finally:
            pr.close()
        late = ds.progressive(t.camera_desc(), p)
        try:
            late.step()
            assert lib.rayz_hip_progressive_track_noise(late._h) == capi.ERR_STATE and b"first step" in lib.rayz_hip_last_error()
        finally:
            late.close()
        assert lib.rayz_hip_progressive_track_noise(None) == capi.ERR_STATE
        assert lib.rayz_hip_noise_kat(F32, None, None, 0, 0, None, None, None, None, None) == capi.ERR_BAD_ARG
    finally:
        ds.close()


def test_other_work_between_steps_changes_nothing_and_destroy_is_clean(gpu):
    t = scene(96, 64)
    p = params(t.params(), chunk_spp=16)
    cam = t.camera_desc()
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        want = run(ds, cam, p, [0])
        pr = ds.progressive(cam, p, track_noise=True)
        try:
            other = params(p, samples_per_px=8, seed=99, width=64, height=36)
            while not pr.done:
                pr.step()
                scratch = out_tensor(other)
                ds.render_into(cam, other, scratch.data_ptr())  # another render and a query on the scene between steps
                ds.sync()
                ds.gbuffer(cam, p, outputs=("index",))
                ds.query_sync()
            q = pr.noise_state().cpu().numpy()
            assert (bits(q) == bits(want["Q"])).all()
            pr.noise(var=True, rel2=True, summary=False)  # in flight ..
        finally:
            pr.close()  # .. when the handle goes
        s = torch.cuda.Stream()  # and on a stream of the caller's: ordered after the pass on the device
        pr = ds.progressive(cam, p, track_noise=True)
        try:
            pr.step(ALL)
            _, var, _ = pr.noise(var=True, summary=False, stream=s.cuda_stream)
            s.synchronize()
            assert (bits32(var.cpu().numpy()) == bits32(want["var"])).all()
        finally:
            pr.close()
    finally:
        ds.close()
