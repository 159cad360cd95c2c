"""Adaptive passes at the sizes where the ordered compaction's scan turns over (DESIGN.md §4.14 "Device side").

adaptive_scan_kernel is one workgroup over one survivor count per block of 256 list entries: a scan within a wave of 64 counts,
a sum over the earlier waves (more than 64 blocks: more than 16,384 entries) and a carry over rounds of 1,024 counts (more than
262,144 entries).  tests/test_adaptive_gpu.py stays within 21 blocks; here rayz_hip_adaptive_kat runs tests/adaptive_masks.py's
designed freeze maps at 16,384 .. 524,545 entries, every value bit for bit against adaptive_ref and every list against the lists
the map alone gives, and an adaptive handle renders 192x108 (81 blocks) and 704x396 (1,089 blocks) against plain handles.
tests/test_adaptive_masks_cpu.py shows on a model which misreading of the kernels each case would catch."""
import numpy as np
import pytest

import adaptive_masks as masks
import adaptive_ref
from test_adaptive_gpu import BVH, F32, F64, REL_ERROR, check_against_plain, out_tensor, params, plain_steps, same, scene

pytestmark = pytest.mark.gpu

KAT_CASES = [(F32,) + c for c in masks.CASES] + [(F64, n, 0, "random") for n in masks.F64_SIZES]
KAT_IDS = ["f32-" + i for i in masks.CASE_IDS] + [f"f64-{n}-random" for n in masks.F64_SIZES]


@pytest.mark.parametrize("prec, n, width, name", KAT_CASES, ids=KAT_IDS)
def test_kat_matches_the_designed_map_at_sizes_that_reach_wave_sums_and_carry(gpu, prec, n, width, name):
    c = masks.case(n, width, name)
    prm = {"rel_error": 0.05, "mean_floor": 0.02, "min_chunks": masks.MIN_CHUNKS, "width": width}
    got = gpu.adaptive_kat(c["sums"], c["sizes"], c["ends"], prec, **prm)
    want = adaptive_ref.run(c["sums"], c["sizes"], c["ends"], f64=prec == F64, **prm)
    assert np.array_equal(got["frozen_at"], want["frozen_at"]) and np.array_equal(got["frozen_at"], c["F"])
    same(got["acc"], want["acc"], "acc")
    same(got["Q"], want["Q"], "Q")
    same(got["frame"], want["frame"], "frame")
    assert len(got["lists"]) == c["K"] + 1
    for p, (g, w) in enumerate(zip(got["lists"], c["lists"])):
        assert len(g) == len(w), f"active list {p}: {len(g)} entries, {len(w)} expected"
        assert np.array_equal(g, w), f"active list {p}: first difference at entry {int(np.argmax(g != w))}"
    for p, end in enumerate(c["ends"]):  # each list is the ordered compaction of the one before, by the device's own frozen_at
        cur = got["lists"][p]
        f = got["frozen_at"][cur]
        assert np.array_equal(got["lists"][p + 1], cur[(f == 0) | (f > end)]), f"pass {p}"
    # the case went where it claims: pass 1 compacts a list beyond the threshold into one that is neither empty nor whole
    before, after = len(got["lists"][1]), len(got["lists"][2])
    assert before == n > masks.claim(n)
    assert after == n if name == "nobody_freezes" else 0 < after < before


@pytest.mark.parametrize("width", [192, 704])
def test_a_rendered_frame_equals_plain_handles_beyond_one_wave_and_one_round(gpu, width):
    """randomBouncing at 192x108 (20,736 pixels, 81 blocks: two waves of the scan) and at 704x396 (278,784 pixels, 1,089 blocks: two
    rounds), f32 through the BVH (adaptive_pass_kernel_bvh and the handle's own buffers), 32 spp in chunks of 8, a pass per chunk,
    min_chunks 2, rel_error 0.0625: frozen_at, frame and counts against the plain tracked handle at every boundary, the active
    count after every pass, and the handle's noise() and noise_rgb() against the plain handle's at the boundary each pixel froze
    at.  The frame must be a mix: at least 10 % of the pixels frozen before the end and at least 1 % never.  The plain handle's
    own estimate gives, at these settings, 8,742 of 20,736 (42.2 %) and 11,664 (56.3 %) at 192x108, 120,969 of 278,784 (43.4 %)
    and 152,121 (54.6 %) at 704x396; the lists after the four passes hold 278,784 / 167,089 / 157,815 / 152,121 entries there."""
    t = scene(width, 32, F32, BVH)
    p = params(t.params(), chunk_spp=8)
    cam, n = t.camera_desc(), width * (width * 9 // 16)
    ds = gpu.DeviceScene(t.scene_desc())
    try:
        one_shot = out_tensor(p)
        ds.render_into(cam, p, one_shot.data_ptr())
        ds.sync()
        one_shot = one_shot.cpu().numpy()
        plain = plain_steps(ds, cam, p, min_samples=8, rel_error=REL_ERROR, rgb=True)
        pr = ds.progressive(cam, p, adaptive=True, min_chunks=2)
        out, sms = out_tensor(p), []
        while True:
            sms.append(pr.adaptive_step(rel_error=REL_ERROR, min_samples=8, out=out))
            if sms[-1].active == 0 or pr.done:
                break
        _, var, rel2 = pr.noise(rel_error=REL_ERROR, var=True, rel2=True)
        v3 = pr.noise_rgb()
        stats = pr.stats()
        ad = {"frame": out.cpu().numpy(), "frozen_at": pr.frozen_at().cpu().numpy(), "counts": pr.sample_counts().cpu().numpy(),
              "summaries": sms, "stats": stats, "chunks_done": pr.chunks_done}
        var, rel2, v3 = var.cpu().numpy(), rel2.cpu().numpy(), v3.cpu().numpy()
        pr.close()
    finally:
        ds.close()
    assert ad["frozen_at"].size == n and sorted(plain) == [1, 2, 3, 4] and ad["chunks_done"] == 4
    first = check_against_plain(ad, plain, one_shot, p, 2, f"{width} wide")
    active = [np.count_nonzero((first == 0) | (first > k)) for k in (1, 2, 3, 4)]
    assert [s.active for s in sms] == active and [s.chunks_done for s in sms] == [1, 2, 3, 4]
    early, never = np.count_nonzero((first != 0) & (first < 4)), np.count_nonzero(first == 0)
    print(f"{width} wide: {early} of {n} pixels freeze before the end, {never} never freeze; active after each pass {active}")
    assert active[0] == n > masks.claim(n) >= masks.WAVE_ENTRIES and 0 < active[1] < n  # the pass that compacts the whole list
    assert early >= 0.10 * n and never >= 0.01 * n, (early, never)
    K = np.where(first != 0, first, 4)
    for k in np.unique(K):
        m = K == k
        same(var[m], plain[k][1][m], f"var at K = {k}")
        same(rel2[m], plain[k][2][m], f"rel2 at K = {k}")
        same(v3[m], plain[k][3][m], f"var_rgb at K = {k}")
