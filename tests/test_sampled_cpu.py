"""Sampled G-buffers (rayz_hip_scene_query_camera_sampled) without a GPU: the contract's restatement
(sampled_ref on the oracle backend) shows, on the frames of sampled_scenes, every case the GPU test relies on; its path ids are the
render's (oracle.render_b with max_bounces = 1); it meets hand-derived cases; QueryResult.with_albedo checks its argument; and the
entry's refusals are made before any HIP call."""
import ctypes as C

import numpy as np
import pytest

import sampled_ref
import sampled_scenes as ss
from rayz_amd import capi, render, tracer

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64


@pytest.fixture(scope="module")
def tracers():
    return {c: ss.build(c) for c in ss.CAMERAS}


@pytest.fixture(scope="module")
def frames(oracle, tracers):
    """rec(camera, precision, width, height): every sample's record of the whole frame, each computed once."""
    done = {}

    def rec(cam, precision, width=ss.W, height=ss.H):
        key = (cam, precision, width, height)
        if key not in done:
            t = tracers[cam]
            be = sampled_ref.OracleBackend(oracle, t.scene_desc(), precision)
            px, py = ss.shape_pixels(width, height)
            done[key] = sampled_ref.records(be, oracle, t.camera_desc(), px, py, width, ss.SPP, ss.SEED, ss.TMIN)
        return done[key]

    return rec


@pytest.mark.parametrize("precision", [F32, F64], ids=["f32", "f64"])
def test_the_frames_show_every_case(frames, precision):
    """.. and no path of any test frame needs more draws than RAYZ_KAT_GET_RAY's list holds (records() asserts it for every pixel
    and sample, both widths, both cameras)."""
    for width, height in ((ss.W, ss.H), (50, 37)):
        n = {}
        for cam in ss.CAMERAS:
            r = frames(cam, precision, width, height)
            assert int(r["draws"].max()) <= sampled_ref.MAX_DRAWS
            assert (r["draws"] == 3).all() if cam == "pinhole" else ((r["draws"] >= 5) & (r["draws"] % 2 == 1)).all()
            for k, v in ss.classes(r, ss.SPP).items():
                n[(cam, k)] = v
        print(width, height, n)
        for cam in ss.CAMERAS:
            for k in ("hits = n", "hits = 0", "0 < hits < n", "two hittables", "moving sphere hit by some samples", "all on the triangle",
                      "all on glass", "both checker colours"):
                assert n[(cam, k)] > 0, (width, height, cam, k, n)
        assert n[("lens", "samples with more than one lens try")] > 0
    # the lens blurs the near sphere's silhouette: more pixels see it in some samples only than through the pinhole
    mixed = {cam: int(((frames(cam, precision)["index"] == ss.NEAR).any(axis=1) & ~(frames(cam, precision)["index"] == ss.NEAR).all(axis=1)).sum())
             for cam in ss.CAMERAS}
    assert mixed["lens"] > mixed["pinhole"] > 0, mixed
    # means of pixels that lie on the triangle or on glass in every sample: a glass albedo is exactly 1
    r = frames("lens", precision)
    m = sampled_ref.means(r, ss.SPP, precision)
    glass = (r["index"] == ss.GLASS).all(axis=1)
    assert (m["albedo"][glass] == 1.0).all() and (m["hits"][glass] == ss.SPP).all()


@pytest.mark.parametrize("n", [1, 3])
def test_the_path_ids_are_the_renders(oracle, tracers, n):
    """A render of the same params with max_bounces = 1 and samples_per_px = n: a path that hits ends at the bounce limit and
    contributes nothing, a miss contributes the sky — so a pixel is (0, 0, 0) exactly where every one of the n samples hits."""
    t = tracers["lens"]
    sd, cam = t.scene_desc(), t.camera_desc()
    # the premise, on the oracle: inside a sphere everything is black, in an empty scene nothing is
    inside = tracer.Tracer.init(8, 40.0, 1.0, 0.0, (0, 0, 0), (0, 0, -1), (0, 1, 0), seed=1)
    inside.pool.add_sphere((0, 0, 0), 5.0, inside.pool.add_diffuse(inside.pool.add_solid_texture((0.5, 0.5, 0.5))))
    empty = tracer.Tracer.init(8, 40.0, 1.0, 0.0, (0, 0, 0), (0, 0, -1), (0, 1, 0), seed=1)
    for tr, black in ((inside, True), (empty, False)):
        p = ss.frame_params(tr, F32, capi.TRAVERSAL_LINEAR, 8, 5, spp=n)
        img, _ = oracle.render_b(tr.scene_desc(), tr.camera_desc(), p)
        assert (img == 0).all() if black else (img > 0).all()
    for precision in (F32, F64):
        p = ss.frame_params(t, precision, capi.TRAVERSAL_LINEAR, spp=n)
        assert p.max_bounces == 1
        img, _ = oracle.render_b(sd, cam, p)
        px, py = ss.shape_pixels(ss.W, ss.H)
        be = sampled_ref.OracleBackend(oracle, sd, precision)
        rec = sampled_ref.records(be, oracle, cam, px, py, ss.W, n, ss.SEED, ss.TMIN)
        hits = sampled_ref.means(rec, n, precision)["hits"].reshape(ss.H, ss.W)
        black = (img == 0).all(axis=2)
        assert np.array_equal(black, hits == n) and (img[~black] > 0).all(axis=1).all()
        assert 0 < int(black.sum()) < black.size
        assert n == 1 or int(((hits > 0) & (hits < n)).sum()) > 0


# ---- hand cases -------------------------------------------------------------------------------------------------------------
def _small(build=None):
    t = tracer.Tracer.init(8, 40.0, 2.0, 2.0, (0, 0, 0), (0, 0, -1), (0, 1, 0), seed=1)
    if build:
        build(t.pool)
    return t


@pytest.mark.parametrize("precision", [F32, F64], ids=["f32", "f64"])
def test_hand_cases(oracle, precision):
    px, py = ss.shape_pixels(8, 5)
    # an empty scene: every sample misses
    t = _small()
    be = sampled_ref.OracleBackend(oracle, t.scene_desc(), precision)
    rec = sampled_ref.records(be, oracle, t.camera_desc(), px, py, 8, 5, 11, ss.TMIN)
    for n in (1, 3, 5):
        m = sampled_ref.means(rec, n, precision)
        assert (m["albedo"] == 1.0).all() and (m["normal"] == 0.0).all() and not np.signbit(m["normal"]).any()
        assert (m["t"] == np.inf).all() and (m["hits"] == 0).all()
    # one solid sphere enclosing the camera: every sample hits, from inside; the albedo's mean is the colour where n·c / n = c
    col = (0.5, 0.25, 0.75)
    t = _small(lambda P: P.add_sphere((0, 0, 0), 5.0, P.add_diffuse(P.add_solid_texture(col))))
    be = sampled_ref.OracleBackend(oracle, t.scene_desc(), precision)
    rec = sampled_ref.records(be, oracle, t.camera_desc(), px, py, 8, 5, 11, ss.TMIN)
    # (t counts in lengths of d; the lens disk is 0.035 wide, so every origin is that near the centre of the sphere of radius 5)
    assert (np.abs(rec["t"] * np.linalg.norm(rec["rays"][:, :, 4:7], axis=2) - 5.0) < 0.04).all()
    for n in (1, 3, 5):
        m = sampled_ref.means(rec, n, precision)
        assert (m["hits"] == n).all() and np.isfinite(m["t"]).all()
        assert (m["albedo"] == np.array(col)).all()  # (dyadic colours: k·c is exact for k <= 5)
        assert (m["t"] >= rec["t"][:, :n].min(axis=1) * (1 - 1e-6)).all() and (m["t"] <= rec["t"][:, :n].max(axis=1) * (1 + 1e-6)).all()
        assert (np.linalg.norm(m["normal"], axis=1) <= 1.0 + 1e-6).all()
    # n = 1 is the single record (0 + x and x / 1: x, but for the sign of a zero)
    m = sampled_ref.means(rec, 1, precision)
    assert np.array_equal(m["albedo"], rec["albedo"][:, 0]) and np.array_equal(m["t"], rec["t"][:, 0])
    assert np.array_equal(m["normal"], rec["normal"][:, 0] + 0.0)


# ---- the Python layer and the ABI, without a device -----------------------------------------------------------------------------
def test_with_albedo_checks_its_argument():
    import torch

    g = render.QueryResult()
    g.albedo = torch.zeros((5, 8, 3), dtype=torch.float32)
    g.index = torch.zeros((5, 8), dtype=torch.int32)
    g.normal = torch.zeros((5, 8, 3), dtype=torch.float32)
    a = torch.ones((5, 8, 3), dtype=torch.float32)
    r = g.with_albedo(a)
    assert r is not g and r.albedo is a and g.albedo is not a and r.index is g.index and r.normal is g.normal and r.t is None
    assert r.is_chain == g.is_chain
    for bad in (torch.ones((5, 8, 3), dtype=torch.float64), torch.ones((5, 8), dtype=torch.float32), torch.ones((8, 5, 3), dtype=torch.float32),
                torch.ones((5, 8, 6), dtype=torch.float32)[:, :, ::2], np.ones((5, 8, 3), np.float32)):
        with pytest.raises(ValueError, match="with_albedo"):
            g.with_albedo(bad)
    with pytest.raises(ValueError, match="no albedo"):
        render.QueryResult().with_albedo(a)


def test_sampled_arguments_are_refused_before_any_hip_call(built):
    """On a machine without a GPU a HIP call would fail with NO_DEVICE or ERR_HIP; these are BAD_ARG with their own message."""
    lib = capi.load()
    t = tracer.threeSpheres(32, seed=1)
    sd, cam = t.scene_desc(), t.camera_desc()
    h = C.c_void_p()
    assert lib.rayz_hip_scene_create(C.byref(sd), C.byref(h)) == capi.OK
    try:
        out = capi.SampledOutputs()

        def call(sampled, params, outputs=out, camera=cam, scene=h):
            return lib.rayz_hip_scene_query_camera_sampled(scene, C.byref(camera) if camera else None, C.byref(params) if params else None,
                                                           C.byref(sampled) if sampled else None, C.byref(outputs) if outputs else None, None)

        def params(**kw):
            p = t.params()
            p.samples_per_px = 4
            for k, v in kw.items():
                setattr(p, k, v)
            return p

        assert call(capi.SampledParams(samples=5), params()) == capi.ERR_BAD_ARG
        assert b"samples 5 > samples_per_px 4" in lib.rayz_hip_last_error()
        for sp in (None, capi.SampledParams(samples=0), capi.SampledParams(samples=1)):
            assert call(sp, params(samples_per_px=0)) == capi.ERR_BAD_ARG
            assert b"samples_per_px must be > 0" in lib.rayz_hip_last_error()
        assert call(capi.SampledParams(samples=2), params(), outputs=None) == capi.ERR_BAD_ARG
        assert b"outputs is null" in lib.rayz_hip_last_error()
        # what the chain call refuses
        assert call(None, None) == capi.ERR_BAD_ARG and b"params is null" in lib.rayz_hip_last_error()
        assert call(None, params(), camera=None) == capi.ERR_BAD_ARG and b"camera is null" in lib.rayz_hip_last_error()
        assert call(None, params(), scene=None) == capi.ERR_BAD_ARG and b"scene handle is null" in lib.rayz_hip_last_error()
        assert call(None, params(precision=9)) == capi.ERR_BAD_ARG and b"precision" in lib.rayz_hip_last_error()
        assert call(None, params(traversal=9)) == capi.ERR_BAD_ARG and b"traversal" in lib.rayz_hip_last_error()
        assert call(None, params(tmin=float("nan"))) == capi.ERR_BAD_ARG and b"tmin" in lib.rayz_hip_last_error()
        assert call(None, params(width=0)) == capi.ERR_BAD_ARG and b"width" in lib.rayz_hip_last_error()
        assert call(None, params(shard_index=2, shard_count=2)) == capi.ERR_BAD_ARG and b"shard_index" in lib.rayz_hip_last_error()
        # accepted arguments get as far as the device (none here: not BAD_ARG), NULL params or samples = 0 meaning n = spp
        import torch

        if not torch.cuda.is_available():
            assert call(None, params()) not in (capi.OK, capi.ERR_BAD_ARG)
            assert call(capi.SampledParams(samples=4), params()) not in (capi.OK, capi.ERR_BAD_ARG)
    finally:
        assert lib.rayz_hip_scene_destroy(h) == capi.OK
