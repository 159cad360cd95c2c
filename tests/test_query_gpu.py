"""Ray queries (rayz_hip_scene_query*, `DeviceScene.query / gbuffer / pick`) on the GPU, held to the oracle exactly.

Each ray's result must be the brute-force `findHit` over every primitive through the oracle's mode-B known-answer pieces
(tests/query_reference.py): index and t exactly, for sphere winners the hit record exactly, material and albedo from the pool
and its checker chain; the BVH and the flat list must agree in every field; ANY must be exactly NEAREST's `index >= 0`."""
import numpy as np
import pytest
import torch

from helpers import assert_images_equal
from query_reference import SCENES, TMIN, albedo_of, brute_force, narrow, pool_arrays, ray_mix
from rayz_amd import capi, render, tracer

pytestmark = pytest.mark.gpu

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR, BVH, AUTO = capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH, capi.TRAVERSAL_AUTO


def run_query(ds, rays, precision, traversal, kind="nearest"):
    dt = torch.float64 if precision == F64 else torch.float32
    r = ds.query(torch.tensor(rays, dtype=dt, device="cuda"), tmin=TMIN, kind=kind, traversal=traversal)
    ds.query_sync()
    return {k: getattr(r, k).cpu().numpy() for k in render.QUERY_OUTPUTS + ("hit",) if getattr(r, k) is not None}


def check_against_oracle(oracle, sd, want, got, precision):
    idx, tt, rec, _ = want
    assert np.array_equal(got["index"], idx), f"index differs on {int((got['index'] != idx).sum())} of {len(idx)} rays"
    assert np.array_equal(got["t"].astype(np.float64), tt)
    ns = sd.n_spheres
    sph = np.nonzero((idx >= 0) & (idx < ns))[0]
    assert (rec[sph, 9] == 1.0).all()  # no winner was filtered out
    assert np.array_equal(got["point"][sph].astype(np.float64), rec[sph, 2:5])
    assert np.array_equal(got["normal"][sph].astype(np.float64), rec[sph, 5:8])
    assert np.array_equal(got["front_face"][sph].astype(np.float64), rec[sph, 8])
    miss = idx < 0
    assert (got["material"][miss] == -1).all() and (got["point"][miss] == 0).all() and (got["front_face"][miss] == 0).all()
    _, _, _, smat, _, tmat = pool_arrays(sd)
    allmat = np.concatenate([smat, tmat])
    hit = np.nonzero(idx >= 0)[0]
    assert np.array_equal(got["material"][hit], allmat[idx[hit]])
    for j in hit[:: max(1, len(hit) // 400)]:  # (the albedo walk is a host loop: a sample of the winners)
        want = albedo_of(oracle, sd, int(allmat[idx[j]]), got["point"][j].astype(np.float64), precision)
        assert np.array_equal(got["albedo"][j].astype(np.float64), want), (j, got["albedo"][j], want)
    return idx


@pytest.mark.parametrize("precision", [F32, F64])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_query_matches_the_oracle_bit_for_bit(gpu, oracle, name, precision):
    t = SCENES[name]()
    sd = t.scene_desc()
    ds = render.DeviceScene(sd)
    rays = ray_mix(oracle, t, precision, 1024, seed=sum(map(ord, name)))
    want = brute_force(oracle, sd, rays, TMIN, precision)
    for traversal in (LINEAR, BVH, AUTO):
        got = run_query(ds, rays, precision, traversal)
        check_against_oracle(oracle, sd, want, got, precision)
        # ANY is exactly NEAREST's index >= 0 for the same rays and tmax
        anyr = run_query(ds, rays, precision, traversal, kind="any")
        assert np.array_equal(anyr["hit"], (got["index"] >= 0).astype(np.uint8))
    ds.close()


@pytest.mark.parametrize("which", ["config3", "config5"])
def test_bvh_and_flat_list_agree_on_a_million_rays(gpu, which):
    t = tracer.randomBouncing(1280, -50, 50, seed=42) if which == "config3" else tracer.triangleMesh(1280, 224, seed=1)
    ds = render.DeviceScene(t.scene_desc())
    p = t.params()
    p.width, p.height = 1280, 800
    outs = {}
    for traversal in (BVH, LINEAR):
        p.traversal = traversal
        g = ds.gbuffer(t.camera_desc(), p)
        ds.query_sync()
        outs[traversal] = {k: getattr(g, k).cpu().numpy() for k in render.QUERY_OUTPUTS}
    for k in render.QUERY_OUTPUTS:
        assert np.array_equal(outs[BVH][k], outs[LINEAR][k], equal_nan=True), k
    assert outs[BVH]["index"].size >= 10 ** 6 and (outs[BVH]["index"] >= 0).mean() > 0.3
    ds.close()


def _root_gap(sd, rays, idx):
    """Distance between the two roots of each ray's winning sphere (f64; +inf for a triangle or a miss)."""
    c, v, r, _, _, _ = pool_arrays(sd)
    gap = np.full(len(idx), np.inf)
    s = np.nonzero((idx >= 0) & (idx < len(c)))[0]
    k = idx[s]
    o, d, tm = rays[s, 0:3], rays[s, 4:7], rays[s, 3]
    q = c[k] + v[k] * tm[:, None] - o
    a = (d * d).sum(axis=1)
    hb = (d * q).sum(axis=1)
    disc = hb * hb - a * ((q * q).sum(axis=1) - r[k] * r[k])
    gap[s] = 2.0 * np.sqrt(np.maximum(disc, 0.0)) / a
    return gap


def test_f64_query_agrees_with_mode_a_where_roots_are_separable(gpu, oracle):
    """Mode A (the reference's own functions, f64) decides the same hittable as the F64 query on every ray whose nearest roots are
    separable: the winner's two roots (of either side) and the nearest root of the next hittable more than 1e-6 apart, and no
    finite tmax placed on a root (the rays built with tmax = mode B's root are left out)."""
    t = tracer.randomBouncing(48, -3, 3, seed=9)
    sd = t.scene_desc()
    ds = render.DeviceScene(sd)
    rays = ray_mix(oracle, t, F64, 1024, seed=4)
    got = run_query(ds, rays, F64, BVH)
    ia, ta, _, second = brute_force(oracle, sd, rays, TMIN, F64, mode="a")
    with np.errstate(invalid="ignore"):
        near = np.where(np.isfinite(ta), np.abs(second - ta) <= 1e-6 * np.maximum(1.0, np.abs(ta)), False)
    sep = ~near & np.isinf(rays[:, 7]) & (_root_gap(sd, rays, ia) > 1e-6) & (_root_gap(sd, rays, got["index"].astype(np.int64)) > 1e-6)
    assert sep.mean() > 0.5
    assert np.array_equal(got["index"][sep], ia[sep]), int((got["index"][sep] != ia[sep]).sum())
    ds.close()


@pytest.mark.parametrize("precision", [F32, F64])
def test_camera_form(gpu, oracle, precision):
    t = tracer.randomBouncing(64, -4, 4, seed=13)
    sd, cam = t.scene_desc(), t.camera_desc()
    ds = render.DeviceScene(sd)
    p = t.params()
    p.precision, p.traversal, p.tmin = precision, BVH, TMIN
    w, h = p.width, p.height
    g = ds.gbuffer(cam, p)
    ds.query_sync()
    whole = {k: getattr(g, k).cpu().numpy() for k in render.QUERY_OUTPUTS}
    # its rays are getRay(px, py, null): the same answers as query() on RAYZ_KAT_GET_RAY (n_u = -1) of every pixel
    px, py = np.meshgrid(np.arange(w), np.arange(h))
    rec = np.zeros((w * h, capi.KAT_IN_STRIDE))
    for k, f in enumerate([cam.look_from, cam.px_du, cam.px_dv, cam.px_origin, cam.defocus_u, cam.defocus_v]):
        rec[:, 3 * k:3 * k + 3] = list(f)
    rec[:, 18], rec[:, 19], rec[:, 20], rec[:, 21] = cam.defocus, px.ravel(), py.ravel(), -1
    kr = render.kat(capi.KAT_GET_RAY, rec, precision)
    assert np.array_equal(kr, oracle.kat_b(capi.KAT_GET_RAY, rec, precision))
    rays = np.zeros((w * h, 8))
    rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7] = kr[:, 0:3], kr[:, 3:6], kr[:, 6], np.inf
    got = run_query(ds, rays, precision, BVH)
    for k in render.QUERY_OUTPUTS:
        assert np.array_equal(whole[k].reshape(got[k].shape), got[k]), k
    # a shard's rows are the whole frame's rows
    for si in range(3):
        ps = capi.RenderParams.from_buffer_copy(p)
        ps.shard_index, ps.shard_count, ps.tile_rows = si, 3, 4
        gs = ds.gbuffer(cam, ps)
        ds.query_sync()
        rows = render.shard_row_indices(h, 4, si, 3)
        for k in render.QUERY_OUTPUTS:
            assert np.array_equal(getattr(gs, k).cpu().numpy(), whole[k][rows]), (si, k)
    # pick: the index under one pixel
    for (x, y) in [(0, 0), (w // 2, h // 2), (w - 1, h - 1), (5, h - 3)]:
        assert ds.pick(cam, p, x, y) == whole["index"][y, x]
    ds.close()


@pytest.mark.parametrize("precision", [F32, F64])
def test_far_origins_find_every_grazing_hit(gpu, oracle, precision):
    """A scene first used with a near camera (its reject radii and boxes padded for that), then a batch whose origins lie 20,000
    units out, aimed just inside sphere silhouettes: every hit the brute force finds must be found (the bound step re-pads)."""
    # no ground sphere: a pool of small spheres near the origin keeps the scene's own bound (and its padding) small
    rng = np.random.default_rng(3)
    t = tracer.Tracer.init(32, 40.0, 10.0, 0.0, (0.0, 2.0, 9.0), (0.0, 0.0, 0.0), (0, 1, 0), seed=1)
    P = t.pool
    mat = P.add_diffuse(P.add_solid_texture((0.5, 0.5, 0.5)))
    for _ in range(64):
        P.add_sphere(tuple(rng.uniform(-4, 4, 3)), float(rng.uniform(0.1, 0.6)), mat)
    sd, cam = t.scene_desc(), t.camera_desc()
    ds = render.DeviceScene(sd)
    p = t.params()
    p.precision, p.tmin = precision, TMIN
    ds.gbuffer(cam, p)  # pads the scene for the near camera
    ds.query_sync()
    c, v, r, _, _, _ = pool_arrays(sd)
    m = 4096
    k = rng.integers(0, len(c), m)
    u = rng.normal(size=(m, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = c[k] + 20000.0 * u
    perp = np.cross(u, rng.normal(size=(m, 3)))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    target = c[k] + perp * (r[k] * (1.0 - rng.uniform(0, 2e-4, m)))[:, None]
    rays = narrow(np.concatenate([o, np.zeros((m, 1)), target - o, np.full((m, 1), np.inf)], axis=1), precision)
    idx, tt, _, _ = brute_force(oracle, sd, rays, TMIN, precision)
    assert (idx >= 0).mean() > 0.2
    for traversal in (LINEAR, BVH):
        got = run_query(ds, rays, precision, traversal)
        assert np.array_equal(got["index"], idx), (traversal, int(((idx >= 0) & (got["index"] < 0)).sum()), "grazing hits missed")
        assert np.array_equal(got["t"].astype(np.float64), tt)
    ds.close()


def test_refusals_leave_the_scene_usable(gpu, oracle):
    t = tracer.threeSpheres(32, seed=1)
    ds = render.DeviceScene(t.scene_desc())
    good = np.array([[0, 1, 3, 0.5, 0, 0, -1, np.inf]])
    for bad, what in [((0, 3), 1.5), ((0, 0), float("nan")), ((0, 4), 0.0), ((0, 1), 2e9)]:
        rays = np.repeat(good, 3, axis=0)
        rays[1, bad[1]] = what
        if bad[1] == 4:
            rays[1, 4:7] = 0.0
        with pytest.raises(capi.RayzHipError, match=r"status -1"):
            ds.query(torch.tensor(rays, dtype=torch.float32, device="cuda"))
    got = run_query(ds, np.repeat(good, 3, axis=0), F32, AUTO)
    idx, _, _, _ = brute_force(oracle, t.scene_desc(), np.repeat(good, 3, axis=0), TMIN, F32)
    assert np.array_equal(got["index"], idx)
    ds.close()


BIG = 2 ** 19 + 1  # more than 512 rays per CU on any device of up to 1,024 CUs: query_bounds_kernel's grid-stride loop takes a second trip
# Every refusal query_bounds names: (what it is, the columns patched, their value, what the message must say)
REFUSALS = [("a NaN origin", [0], float("nan"), "NaN or infinite origin, direction or time"),
            ("an infinite direction", [5], float("inf"), "NaN or infinite origin, direction or time"),
            ("a zero direction", [4, 5, 6], 0.0, "a zero direction"),
            ("an origin beyond the limit", [1], 2e9, "beyond RAYZ_QUERY_MAX_ORIGIN"),
            ("a direction below the scale", [4, 5, 6], -1e-12, "RAYZ_QUERY_MIN_DIR"),
            ("a direction above the scale", [6], -1e10, "RAYZ_QUERY_MAX_DIR"),
            ("a NaN tmax", [7], float("nan"), "a NaN tmax"),
            ("time 1.5", [3], 1.5, r"time 1\.5 outside \[0, 1\]"),
            ("time -0.5", [3], -0.5, r"time -0\.5 outside \[0, 1\]")]


def test_a_refusal_is_found_anywhere_in_a_large_batch(gpu, oracle):
    """One bad ray among 2^19 + 1 valid ones, in the last lane of a wave and the first of the next (63, 64), in the last thread of
    a block and the first of the next (255, 256), deep in the grid (2^17), and in the last two rays (2^19 − 1; 2^19, which any grid
    of up to 2,048 blocks reaches only on a second trip of its loop): the flag has to survive the loop, the shuffle, the LDS step
    and the atomic from wherever it is raised.  The batch is built once on the device and one row is patched per run.  The clean
    batch is then accepted: its first three rays are the 3-ray batch of test_refusals_leave_the_scene_usable and answer as that
    does, and a sample of the jittered rest answers as the brute force."""
    t = tracer.threeSpheres(32, seed=1)
    sd = t.scene_desc()
    ds = render.DeviceScene(sd)
    good = np.array([0, 1, 3, 0.5, 0, 0, -1, np.inf])
    rng = np.random.default_rng(19)
    rays = np.tile(good, (BIG, 1))
    rays[3:, 0:3] += rng.uniform(-0.25, 0.25, (BIG - 3, 3))
    rays[3:, 3] = rng.uniform(0, 1, BIG - 3)
    rays[3:, 4:6] += rng.uniform(-0.25, 0.25, (BIG - 3, 2))
    rays = narrow(rays, F32)
    clean = torch.tensor(rays, dtype=torch.float32, device="cuda")
    batch = clean.clone()
    for at in (63, 64, 255, 256, 2 ** 17, 2 ** 19 - 1, 2 ** 19):
        for what, cols, value, says in REFUSALS:
            batch[at, cols] = value
            with pytest.raises(capi.RayzHipError, match=rf"status {capi.ERR_BAD_ARG}\): query rays: .*{says}"):
                ds.query(batch, tmin=TMIN, outputs=("index",))
                pytest.fail(f"{what} at ray {at} of {BIG} was accepted")
            batch[at] = clean[at]
    assert torch.equal(batch, clean)
    r = ds.query(batch, tmin=TMIN)
    ds.query_sync()
    got = {k: getattr(r, k).cpu().numpy() for k in render.QUERY_OUTPUTS}
    small = run_query(ds, rays[:3], F32, AUTO)
    for k in render.QUERY_OUTPUTS:
        assert np.array_equal(got[k][:3], small[k], equal_nan=True), k
    sample = np.concatenate([np.arange(0, BIG, 1021), [BIG - 1]])
    idx, tt, _, _ = brute_force(oracle, sd, rays[sample], TMIN, F32)
    assert np.array_equal(got["index"][sample], idx) and np.array_equal(got["t"][sample].astype(np.float64), tt)
    assert np.array_equal(small["index"], idx[:1].repeat(3)) and (idx >= 0).any()
    ds.close()


def _frame(ds, cam, p):
    out = torch.full((render.shard_rows(p), p.width, 3), float("nan"), device="cuda")
    torch.cuda.synchronize()
    ds.render_into(cam, p, out.data_ptr())
    st = ds.sync()
    return out.cpu().numpy(), (st.primary_rays, st.segments, st.sphere_tests, st.node_tests)


def _render_scene():
    t = tracer.randomBouncing(48, -4, 4, seed=21)
    t.samples_per_px, t.max_bounces = 16, 6
    t.set_gpu(render_seed=5, chunk_spp=4)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    p.traversal = BVH
    return t, sd, cam, p


def test_queries_do_not_disturb_renders(gpu):
    """Render, queries from near the camera, render: the same frame and the same counters, all four; queries between the passes of
    a progressive render: the one-shot frame."""
    t, sd, cam, p = _render_scene()
    ds = render.DeviceScene(sd)
    rng = np.random.default_rng(8)
    near = np.concatenate([np.tile(0.5 * np.array(list(cam.look_from)), (256, 1)), rng.uniform(0, 1, (256, 1)),
                           rng.normal(size=(256, 3)), np.full((256, 1), np.inf)], axis=1)
    near = torch.tensor(near, dtype=torch.float32, device="cuda")
    a, sa = _frame(ds, cam, p)
    ds.query(near)
    ds.gbuffer(cam, p)
    ds.query_sync()
    # the counters of the last render stand, queries in between
    st = ds.sync()
    assert (st.primary_rays, st.segments, st.sphere_tests, st.node_tests) == sa
    b, sb = _frame(ds, cam, p)
    assert_images_equal(b, a, "render after queries")
    assert sb == sa
    # queries between progressive steps: the one-shot frame at the end
    pr = ds.progressive(cam, p)
    out = torch.full((render.shard_rows(p), p.width, 3), float("nan"), device="cuda")
    torch.cuda.synchronize()
    while not pr.done:
        pr.step(0, out.data_ptr())
        ds.query(near, kind="any")
        ds.query_sync()
    pr.stats()
    assert_images_equal(out.cpu().numpy(), a, "progressive with queries between steps")
    pr.close()
    ds.close()


def test_a_far_query_widens_the_padding_but_changes_no_frame(gpu):
    """A batch 3,000 units out re-pads the scene for good (include/rayz_hip.h): later frames are the same, their rays and segments
    too; only the box and primitive tests may grow."""
    t, sd, cam, p = _render_scene()
    ds = render.DeviceScene(sd)
    far = torch.tensor([[3000.0, 1, 2, 0.25, -1, 0, 0, np.inf]] * 64, dtype=torch.float32, device="cuda")
    a, sa = _frame(ds, cam, p)
    ds.query(far)
    ds.query_sync()
    b, sb = _frame(ds, cam, p)
    assert_images_equal(b, a, "render after a far query")
    assert sb[:2] == sa[:2] and sb[2] >= sa[2] and sb[3] >= sa[3]
    ds.close()


def test_query_tensors_outlive_the_call(gpu, oracle):
    """The rays a query reads may be a temporary (a non-contiguous slice's copy, a tensor nobody keeps): the scene keeps them until
    query_sync, so torch reusing and overwriting freed memory in the meantime changes no result."""
    t = tracer.randomBouncing(48, -3, 3, seed=5)
    sd = t.scene_desc()
    ds = render.DeviceScene(sd)
    rays = ray_mix(oracle, t, F32, 1024, seed=12)
    want = brute_force(oracle, sd, rays, TMIN, F32)[0]
    big = torch.zeros((len(rays), 11), dtype=torch.float32, device="cuda")
    big[:, :8] = torch.tensor(rays, dtype=torch.float32, device="cuda")
    r1 = ds.query(big[:, :8], tmin=TMIN, traversal=BVH, outputs=("index",))  # (non-contiguous: the library reads a copy)
    junk = [torch.full((len(rays), 8), float("nan"), device="cuda") for _ in range(8)]  # (torch may hand the copy's block out)
    ds.query_sync()
    assert np.array_equal(r1.index.cpu().numpy(), want)
    r2 = ds.query(torch.tensor(rays, dtype=torch.float32, device="cuda"), tmin=TMIN, traversal=LINEAR, outputs=("index",))
    junk += [torch.full((len(rays), 8), -1.0, device="cuda") for _ in range(8)]
    ds.query_sync()
    assert np.array_equal(r2.index.cpu().numpy(), want)
    with pytest.raises(ValueError, match="GPU memory"):
        ds.query(torch.tensor(rays, dtype=torch.float32))
    del junk
    ds.close()
