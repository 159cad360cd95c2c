"""The denoiser's surface keys on the GPU (rayz_hip_denoiser_set_keys): all-zero keys are keys off; a frame whose
keys split it into parts equals, part by part and bit for bit, the UNKEYED filter run on each part cropped to its own frame — for
both modes at 5 levels (the LDS and the direct taps, the guided mode's prefilter and variance output); exact single-level cases;
and a keyed chain-guided run end to end."""
import numpy as np
import pytest
import torch

import denoise_cases
import denoise_keys_cases as kc
from rayz_amd import capi, tracer

pytestmark = pytest.mark.gpu
W, H = 77, 45


class Guides:
    """What Denoiser.run reads of a gbuffer, from host arrays; `crop(ys, xs)` is the same frame part as its own frame."""

    def __init__(self, index, normal, point, albedo, rgb, var):
        self.host = dict(index=index, normal=normal, point=point, albedo=albedo, rgb=rgb, var=var)
        for k, v in self.host.items():
            setattr(self, k, None if v is None else torch.tensor(np.ascontiguousarray(v), device="cuda"))
        self.is_chain = False

    def crop(self, ys, xs):
        return Guides(*[None if self.host[k] is None else self.host[k][ys, xs] for k in ("index", "normal", "point", "albedo", "rgb", "var")])


def bits(t):
    return t.contiguous().view(torch.int32)


def run_both(gpu, g, keys):
    """(run, run_guided colour, run_guided variance) of frame `g` at 5 levels, as int32 bit patterns on the host."""
    h, w = g.index.shape
    dn = gpu.Denoiser(w, h)
    try:
        kt = None if keys is None else torch.tensor(np.ascontiguousarray(keys).view(np.int32), device="cuda")
        a = dn.run(g.rgb, g, keys=kt, levels=5)
        b, v = dn.run_guided(g.rgb, g.var, g, var_out=True, keys=kt, levels=5)
        torch.cuda.synchronize()
        return [bits(x).cpu().numpy() for x in (a, b, v)]
    finally:
        dn.close()


@pytest.fixture(scope="module")
def frame(gpu):
    rgb, index, normal, point, albedo = denoise_cases.synthetic(W, H, seed=21)
    var = (np.random.default_rng(5).random((H, W, 3)) * 0.05).astype(np.float32)
    g = Guides(index, normal, point, albedo, rgb, var)
    return g, run_both(gpu, g, None)


def test_all_zero_keys_are_keys_off(gpu, frame):
    g, off = frame
    for k in (np.zeros((H, W), np.uint32), np.full((H, W), 0xDEADBEEF, np.uint32)):  # (.. and so is any one key for all)
        for x, y in zip(run_both(gpu, g, k), off):
            assert np.array_equal(x, y)


def parts_of(xcuts, ycuts):
    xs = [slice(a, b) for a, b in zip([0] + xcuts, xcuts + [W])]
    ys = [slice(a, b) for a, b in zip([0] + ycuts, ycuts + [H])]
    return [(y, x) for y in ys for x in xs]


@pytest.mark.parametrize("xcuts,ycuts", [([13], []), ([32], []), ([], [8]), ([], [29]), ([13], [29]), ([32], [8])],
                         ids=["column 13", "column 32", "row 8", "row 29", "quadrants 13/29", "quadrants 32/8"])
def test_keys_partition_the_frame(gpu, frame, xcuts, ycuts):
    g, off = frame
    parts = parts_of(xcuts, ycuts)
    keys = np.zeros((H, W), np.uint32)
    for n, (ys, xs) in enumerate(parts):
        keys[ys, xs] = [0x80000000, 0, 0x7FC00000, 3][n]  # (as floats: -0.0 == +0.0, and a NaN)
    keyed = run_both(gpu, g, keys)
    assert any(not np.array_equal(x, y) for x, y in zip(keyed, off))  # (the keys do something)
    for ys, xs in parts:
        alone = run_both(gpu, g.crop(ys, xs), None)
        for name, x, y in zip(("run", "run_guided", "run_guided's variance"), keyed, alone):
            bad = np.argwhere(x[ys, xs] != y)
            assert not len(bad), f"{name}: part rows {ys}, columns {xs} differs from its own unkeyed frame at {len(bad)} values, first {bad[0]}"


def test_exact_single_level_cases(gpu):
    for case in kc.cases():
        g = Guides(case.index, case.normal, case.point, None, case.rgb, None)
        h, w = case.index.shape
        dn = gpu.Denoiser(w, h)
        try:
            kt = torch.tensor(case.keys.view(np.int32), device="cuda")
            for lds in (4, 0):  # the LDS taps, the direct taps
                gpu.debug_set(capi.DEBUG_DENOISE_LDS_STRIDE, lds)
                out = dn.run(g.rgb, g, keys=kt, **kc.PARAMS)
                torch.cuda.synchronize()
                case.check(out.cpu().numpy(), f"LDS strides up to {lds}")
        finally:
            gpu.debug_set(capi.DEBUG_DENOISE_LDS_STRIDE, -1)
            dn.close()


def test_keyed_chain_guided_run_end_to_end(gpu):
    """The cover-like scene at 96x54, 16 spp: the keyed chain-guided runs write finite pixels and differ from the first-hit-guided runs
    only where a chain was followed, or within the filter's footprint of such a pixel (5 levels: 2·(1 + 2 + 4 + 8 + 16) = 62 pixels,
    plus 1 for the guided mode's prefilter)."""
    t = tracer.randomBouncing(96, -3, 3, seed=5)
    t.samples_per_px, t.max_bounces = 16, 8
    t.set_gpu(render_seed=17, chunk_spp=2, traversal=capi.TRAVERSAL_BVH, tmin=1e-3)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    ds = gpu.DeviceScene(sd)
    pr = ds.progressive(cam, p, track_noise=True)
    dn = gpu.Denoiser(p.width, p.height)
    try:
        frame = torch.full((p.height, p.width, 3), float("nan"), device="cuda")
        torch.cuda.synchronize()
        while not pr.done:
            pr.step(0, frame.data_ptr())
        var = pr.noise_rgb()
        pr.stats()
        first = ds.gbuffer(cam, p)
        ds.query_sync()
        chain = ds.gbuffer(cam, p, chain=True)
        ds.query_sync()
        assert chain.is_chain and torch.equal(chain.first_index, first.index)
        followed = (chain.depth > 0).cpu().numpy()
        assert 16 <= followed.sum() < followed.size  # the scene has mirror and glass balls, and more than them
        ys, xs = np.nonzero(followed)
        for levels in (5, 2):
            reach = 2 * (2 ** levels - 1) + 1
            near = np.zeros_like(followed)
            for y, x in zip(ys, xs):
                near[max(0, y - reach):y + reach + 1, max(0, x - reach):x + reach + 1] = True
            a = dn.run(frame, first, levels=levels)  # (five outputs, all kept: the runs are asynchronous on the library's stream)
            b = dn.run(frame, chain, levels=levels)  # keys: the chain result's, by default
            c = dn.run_guided(frame, var, first, levels=levels)
            d = dn.run_guided(frame, var, chain, levels=levels)
            e = dn.run(frame, chain, keys=None, levels=levels)  # chain guides without keys: another image again
            torch.cuda.synchronize()
            for name, x, y in (("run", a, b), ("run_guided", c, d)):
                assert torch.isfinite(y).all(), name
                diff = (bits(x) != bits(y)).any(dim=2).cpu().numpy()
                assert diff.any() and not (diff & ~near).any(), (name, levels, int((diff & ~near).sum()))
            assert not torch.equal(bits(e), bits(b))
        # the next run on a first-hit G-buffer is unkeyed again: the default follows the gbuffer
        again = dn.run(frame, first, levels=2)
        torch.cuda.synchronize()
        assert torch.equal(bits(again), bits(a))
    finally:
        dn.close()
        pr.close()
        ds.close()
