"""Handles give their device memory back: every kind of handle is created, used, synchronised and destroyed over and
over, and the device's free memory must not fall.

One warm-up cycle first (the HIP runtime's own first-use allocations, code objects, torch's cached blocks for the tensors
a cycle makes), then free memory is read, K more cycles run, and it is read again.  Each cycle allocates at least A bytes
in buffers the handle owns — a figure taken from the frame's size alone, stated per kind below.  A handle that leaked
only that much would lose K·A; the test asks for a loss below A, so the margin is a factor of K = 12 without any
measured number.  256x256 pixels, 64 samples in chunks of 16 (4 chunk sums of 16 bytes per pixel in f32), on the pool of
test_reuse_gpu.py (400 spheres, 8 triangles)."""
import pytest
import torch

from rayz_amd import capi, render
from test_reuse_gpu import NEAR, camera, params, pool_tracer

pytestmark = pytest.mark.gpu

MiB = 1 << 20
K = 12
W = H = 256


@pytest.fixture(scope="module")
def setup(gpu, oracle):
    t = pool_tracer()
    p = params(t.params(), width=W, height=H, samples_per_px=64, chunk_spp=16, precision=capi.PRECISION_F32)
    out = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    return t.scene_desc(), camera(oracle, NEAR, W, H), p, out


def scene_cycle(scene, cam, p, out):
    """The chunk-sum workspace alone: 256·256 pixels x 4 chunks x 16 B = 4 MiB."""
    ds = render.DeviceScene(scene)
    for traversal in (capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH):
        ds.render_into(cam, params(p, traversal=traversal), out.data_ptr())
        assert ds.sync().segments > 0
    ds.close()


def progressive_cycle(scene, cam, p, out):
    """Two passes of two chunks: a 2 MiB window of chunk sums in the scene + the handle's 1 MiB accumulator = 3 MiB."""
    ds = render.DeviceScene(scene)
    pr = ds.progressive(cam, p)
    passes = 0
    while not pr.done:
        pr.step(32, out.data_ptr())
        passes += 1
    assert passes == 2 and pr.stats().segments > 0
    pr.close()
    ds.close()


def multi_cycle(scene, cam, p, out):
    """Two scenes of 128 rows each: 2 x 2 MiB of chunk sums = 4 MiB (the tiles, `gathered` and `frame` come on top)."""
    m = render.MultiScene(scene, [0, 0], capi.GATHER_PEER_COPY | capi.GATHER_ALLOW_DUPLICATE_DEVICES)
    _, st = m.render(cam, p)
    assert st.segments > 0
    m.close()


def query_denoise_cycle(scene, cam, p, out):
    """The denoiser's five buffers of one 16-byte record per pixel: 5 x 256·256 x 16 B = 5 MiB."""
    ds = render.DeviceScene(scene)
    g = ds.gbuffer(cam, p)
    assert ds.query_sync().primary_rays == W * H
    dn = render.Denoiser(W, H)
    dn.run(out, g, out=out)
    dn.timing()  # (waits for the run)
    dn.close()
    ds.close()


@pytest.mark.parametrize("cycle,A", [(scene_cycle, 4 * MiB), (progressive_cycle, 3 * MiB), (multi_cycle, 4 * MiB),
                                     (query_denoise_cycle, 5 * MiB)], ids=["scene", "progressive", "multi", "query-denoiser"])
def test_handles_give_their_device_memory_back(setup, cycle, A):
    def free_bytes():
        torch.cuda.synchronize()
        return torch.cuda.mem_get_info()[0]

    cycle(*setup)
    before = free_bytes()
    for _ in range(K):
        cycle(*setup)
    after = free_bytes()
    print(f"{cycle.__name__}: free {before} -> {after} B over {K} cycles ({(before - after) / MiB:+.2f} MiB lost; A = {A // MiB} MiB)")
    assert before - after < A, (cycle.__name__, before, after)
