"""The per-channel variance of a tracked progressive handle (rayz_hip_progressive_noise_rgb, `Progressive.noise_rgb`; DESIGN.md
§4.12, §4.13): var_ch = D_ch / ((K - 1) · N), bit for bit against numpy float64 on the handle's own state.

The accumulator has no accessor; the preview a step writes is acc · (1 / N) in the handle's precision, which is exact when N is a
power of two, so the test evaluates at N = 1, 2, 4 and 8 (8 spp in chunks of one sample) and takes M = preview · N."""
import numpy as np
import pytest
import torch

from rayz_amd import capi, render, tracer

pytestmark = pytest.mark.gpu

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
ALL = 0xFFFFFFFF


def handle(prec, spp=8):
    t = tracer.randomBouncing(48, seed=7)  # 48x27
    t.samples_per_px, t.max_bounces = spp, 8
    t.set_gpu(precision=prec, render_seed=11, chunk_spp=1, traversal=capi.TRAVERSAL_BVH)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    return t, render.DeviceScene(sd), cam, p


def want_rgb(M, Q, K, N):
    """§4.12's D_ch with its clamp, over (K - 1) · N, in float64 (numpy fuses nothing), rounded once to float32."""
    if K < 2:
        return np.full(M.shape, np.inf, np.float32)
    with np.errstate(invalid="ignore"):
        D = Q - (M * M) / float(N)
        D = np.where(D < 0.0, 0.0, D)
        return (D / ((float(K) - 1.0) * float(N))).astype(np.float32)


@pytest.mark.parametrize("prec", [F32, F64], ids=["f32", "f64"])
def test_noise_rgb_equals_numpy_on_the_handles_state(gpu, prec):
    t, ds, cam, p = handle(prec)
    dt = torch.float64 if prec == F64 else torch.float32
    one_shot = torch.empty((p.height, p.width, 3), dtype=dt, device="cuda")
    torch.cuda.synchronize()
    ds.render_into(cam, p, one_shot.data_ptr())
    ds.sync()
    pr = ds.progressive(cam, p, track_noise=True)
    preview = torch.full((p.height, p.width, 3), float("nan"), dtype=dt, device="cuda")
    torch.cuda.synchronize()
    seen = []
    for step in (1, 1, 2, ALL):
        pr.step(step, preview.data_ptr())
        var = pr.noise_rgb()
        pr.stats()  # waits for the pass and the evaluation
        K, N = pr.chunks_done, pr.samples_done
        assert K == N and N & (N - 1) == 0
        seen.append(N)
        M = preview.cpu().numpy().astype(np.float64) * N  # = acc, exactly (N a power of two)
        Q = pr.noise_state().cpu().numpy()[..., :3]
        got = var.cpu().numpy()
        assert got.shape == (p.height, p.width, 3) and got.dtype == np.float32
        want = want_rgb(M, Q, K, N)
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        assert len(bad) == 0, f"N={N}: {len(bad)} of {got.size} differ; first at {bad[:3].tolist()}"
        if K < 2:
            assert np.isposinf(got).all()
        else:
            assert np.isfinite(got).all() and (got >= 0).all() and (got > 0).any()
            # the three channels sum to §4.12's `var` up to the order of the roundings
            _, v1, _ = pr.noise(var=True)
            np.testing.assert_allclose(got.astype(np.float64).sum(axis=2), v1.cpu().numpy().astype(np.float64), rtol=1e-6, atol=0)
    assert seen == [1, 2, 4, 8] and pr.done
    # the evaluations in between changed nothing: the last preview is the one-shot frame
    assert torch.equal(preview, one_shot)
    pr.close()
    ds.close()


def test_an_untracked_handle_is_refused(gpu):
    t, ds, cam, p = handle(F32, spp=2)
    pr = ds.progressive(cam, p)
    with pytest.raises(capi.RayzHipError, match="does not track noise"):
        pr.noise_rgb()
    pr.step(ALL)
    with pytest.raises(capi.RayzHipError, match="does not track noise"):
        pr.noise_rgb()
    pr.stats()
    pr.close()
    ds.close()
