"""Ray queries on the GPU held to the exact `findHit` (tests/query_exact.py), not only to the mode-B restatement of their own
arithmetic: every query scene and triangle winners included, triangle-adversarial rays, direction-scale covariance over the
accepted range and its refusal beyond, tmin / tmax edges, the output contract of the C ABI, and the camera form.  The BVH and the
flat list must agree in every field throughout.  Each check prints its unambiguous fraction and its largest error against the
bound (pytest -s)."""
import ctypes as C

import numpy as np
import pytest
import torch

from query_exact import Scene, check_exact, exact_find_hit
from query_reference import SCENES, TMIN, brute_force, narrow, plane_scene, ray_mix
from rayz_amd import capi, render, tracer
from test_query_cpu import _pool
from test_query_gpu import check_against_oracle

pytestmark = pytest.mark.gpu

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR, BVH = capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH
FIELDS = render.QUERY_OUTPUTS


def _run(ds, rays, precision, traversal, tmin=TMIN, kind="nearest"):
    dt = torch.float64 if precision == F64 else torch.float32
    r = ds.query(torch.tensor(rays, dtype=dt, device="cuda"), tmin=tmin, kind=kind, traversal=traversal)
    ds.query_sync()
    return {k: getattr(r, k).cpu().numpy() for k in FIELDS + ("hit",) if getattr(r, k) is not None}


def _both(ds, rays, precision, tmin=TMIN):
    """NEAREST through the flat list and the BVH: identical in every field; ANY = NEAREST's index >= 0 for both."""
    a = _run(ds, rays, precision, LINEAR, tmin)
    b = _run(ds, rays, precision, BVH, tmin)
    for k in FIELDS:
        assert np.array_equal(a[k], b[k]), f"BVH and flat list differ in {k}"
    for trav in (LINEAR, BVH):
        assert np.array_equal(_run(ds, rays, precision, trav, tmin, "any")["hit"], (a["index"] >= 0).astype(np.uint8))
    return a


def _exact(sd, rays, got, precision, tmin=TMIN, what=""):
    S = Scene(sd)
    summary = check_exact(sd, rays, got, exact_find_hit(sd, rays, tmin, precision, S), precision, S)
    print(what, summary)
    return summary


@pytest.mark.parametrize("precision", [F32, F64])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_every_scene_held_to_the_exact_reference(gpu, oracle, name, precision):
    t = SCENES[name]()
    sd = t.scene_desc()
    ds = render.DeviceScene(sd)
    rays = ray_mix(oracle, t, precision, 384, seed=sum(map(ord, name)) + 17)
    got = _both(ds, rays, precision)
    s = _exact(sd, rays, got, precision, what=(name, precision))
    assert s["unambiguous"] >= 0.8
    check_against_oracle(oracle, sd, brute_force(oracle, sd, rays, TMIN, precision), got, precision)
    if sd.n_triangles:
        assert (got["index"] >= sd.n_spheres).mean() > 0.2  # triangle winners are held to their exact records
    ds.close()


def adversarial_triangles():
    """Slivers, a fan of six triangles around one shared vertex, and a pair sharing an edge at coordinates around 1e4."""
    tris = []
    c = np.array([0.3, 0.2, -4.0])
    ring = [c + [np.cos(2 * np.pi * k / 6), np.sin(2 * np.pi * k / 6), 0.1 * (k % 3)] for k in range(6)]
    for k in range(6):
        tris.append((tuple(c), tuple(ring[k]), tuple(ring[(k + 1) % 6])))
    tris.append(((-3.0, -1.0, -6.0), (3.0, -1.0, -6.0), (3.0, -0.999, -6.0)))  # sliver, 6 x 0.001
    tris.append(((-3.0, 1.0, -5.0), (3.0, 1.0, -5.0 + 1e-5), (-3.0, 1.0 + 1e-6, -5.0)))  # thinner
    tris.append(((-2.0, 0.0, -2.0), (2.0, 0.0, -2.0), (0.0, 0.1, 2.0)))  # a floor tile above the ground sphere
    big = np.array([1.0e4, 1.0e4 + 3.0, -1.0e4])
    tris.append((tuple(big), tuple(big + [2.0, 0.0, 0.3]), tuple(big + [0.5, 2.0, 0.0])))
    tris.append((tuple(big + [2.0, 0.0, 0.3]), tuple(big + [2.5, 2.5, 0.1]), tuple(big + [0.5, 2.0, 0.0])))
    return tris


def adversarial_rays(tri, rng, precision, n_each):
    """Rays through vertices (shared in the fan), edge midpoints (shared edges) and centroids from both sides (back faces), and
    rays grazing the triangle planes at 1e-3 to 1e-7 rad (det near 0)."""
    out = []
    for k in rng.integers(0, len(tri), n_each):
        v = tri[k]
        nrm = np.cross(v[1] - v[0], v[2] - v[0])
        nrm /= np.linalg.norm(nrm)
        for target in (v[rng.integers(0, 3)], 0.5 * (v[0] + v[1]), 0.5 * (v[1] + v[2]), (v[0] + v[1] + v[2]) / 3):
            for side in (1.0, -1.0):
                o = target + side * (nrm * rng.uniform(1, 5) + rng.normal(scale=0.7, size=3))
                out.append(np.concatenate([o, [0.0], target - o, [np.inf]]))
        inplane = np.cross(nrm, rng.normal(size=3))
        inplane /= np.linalg.norm(inplane)
        target = (v[0] + v[1] + v[2]) / 3
        for ang in (1e-3, 1e-4, 1e-5, 1e-6, 1e-7):
            d = inplane * np.cos(ang) - nrm * np.sin(ang)
            out.append(np.concatenate([target - 3.0 * d, [0.0], d, [np.inf]]))
    rays = narrow(np.array(out), precision)
    return rays[np.abs(rays[:, 4:7]).sum(axis=1) > 0]


def adversarial_scenes():
    return {"mesh": tracer.triangleMesh(48, 10, seed=1).scene_desc(),
            "hand": _pool([((0.0, -1004.0, 0.0), 1000.0, (0.0, 0.0, 0.0))], adversarial_triangles())}


@pytest.mark.parametrize("precision", [F32, F64])
def test_triangle_adversarial_rays(gpu, precision):
    """Edges, vertices, grazing rays and back faces: the index is always one the exact bounds allow, t / point / normal within the
    bounds, and the f32 BVH boxes (padded by 1e-4 + E) lose no hit the flat list finds."""
    rng = np.random.default_rng(31 + precision)
    for which, sd in adversarial_scenes().items():
        ds = render.DeviceScene(sd)
        rays = adversarial_rays(Scene(sd).tri, rng, precision, 40 if which == "mesh" else 60)
        if which == "hand":
            # first, two whole waves of rays down through the floor tile: every lane also hits the ground sphere behind it, so a
            # flat scan that skipped the triangle stream once all of a wave's lanes have a hit would report the ground
            o = np.concatenate([rng.uniform((-0.3, 4.0, -1.5), (0.3, 6.0, -0.5), (128, 3)), np.zeros((128, 1))], axis=1)
            down = np.concatenate([o, rng.uniform((-0.05, -1.0, -0.05), (0.05, -1.0, 0.05), (128, 3)), np.full((128, 1), np.inf)], axis=1)
            rays = np.concatenate([narrow(down, precision), rays])
        got = _both(ds, rays, precision)
        s = _exact(sd, rays, got, precision, what=(which, precision))
        assert (got["index"] >= sd.n_spheres).mean() > 0.3
        if which == "hand":
            assert (got["index"][:128] == sd.n_spheres + 8).all()  # the tile, in front of the ground
        # (six of the thirteen rays per triangle aim at a vertex or an edge midpoint, where a barycentric is exactly 0, and five
        # graze: ambiguous by construction, held to the allowed set; the centroid rays are not)
        assert s["unambiguous"] >= 0.15
        ds.close()


def covariance_scene():
    """plane_scene(11) — static and y-moving plane runs, loose static / y-moving / generally moving spheres, the r = 1000 ground
    (an oversized hittable) — plus 24 triangles."""
    t = plane_scene(11)
    P = t.pool
    m = P.add_diffuse(P.add_solid_texture((0.3, 0.6, 0.2)))
    rng = np.random.default_rng(4)
    for _ in range(24):
        v0 = rng.uniform((-6, -2, -6), (6, 3, 6))
        P.add_triangle(tuple(v0), tuple(v0 + rng.normal(size=3)), tuple(v0 + rng.normal(size=3)), m)
    return t


@pytest.mark.parametrize("precision", [F32, F64])
def test_direction_scale_covariance_and_its_refusal(gpu, oracle, precision):
    """d·2^k with tmin and tmax·2^-k: the same hittable and every field but t the same, t·2^k = t₀ exactly, for k from -32 to 32
    (max_k |d_k| of the base rays is exactly 1: the ends are RAYZ_QUERY_MIN_DIR and RAYZ_QUERY_MAX_DIR), both traversals, NEAREST
    and ANY.  Just outside the range: RAYZ_ERR_BAD_ARG, and the scene still answers as before."""
    t = covariance_scene()
    sd = t.scene_desc()
    assert sd.n_triangles == 24
    ds = render.DeviceScene(sd)
    rays = ray_mix(oracle, t, precision, 192, seed=77)
    rays[:, 4:7] /= np.abs(rays[:, 4:7]).max(axis=1, keepdims=True)
    rays = narrow(rays, precision)
    assert (np.abs(rays[:, 4:7]).max(axis=1) == 1.0).all()
    dt = torch.float64 if precision == F64 else torch.float32
    base = {trav: _run(ds, rays, precision, trav) for trav in (LINEAR, BVH)}
    assert (base[BVH]["index"] >= 0).mean() > 0.3 and (base[BVH]["index"] >= sd.n_spheres).any()
    for k in sorted(set(range(-32, 33, 8)) | {-31, 31}):
        r2 = rays.copy()
        r2[:, 4:7] *= 2.0 ** k
        r2[:, 7] *= 2.0 ** -k
        for trav in (LINEAR, BVH):
            got = _run(ds, r2, precision, trav, tmin=TMIN * 2.0 ** -k)
            for f in FIELDS:
                if f != "t":
                    assert np.array_equal(got[f], base[trav][f]), (k, trav, f)
            assert np.array_equal(got["t"].astype(np.float64) * 2.0 ** k, base[trav]["t"].astype(np.float64)), (k, trav)
            anyr = _run(ds, r2, precision, trav, tmin=TMIN * 2.0 ** -k, kind="any")
            assert np.array_equal(anyr["hit"], (base[trav]["index"] >= 0).astype(np.uint8)), (k, trav)
    for bad in (2.0 ** 33, 2.0 ** -33, float(np.nextafter(np.float32(2.0 ** 32), np.float32(np.inf))),
                float(np.nextafter(np.float32(2.0 ** -32), np.float32(0)))):
        r2 = rays[:4].copy()
        r2[1, 4:7] = [bad, 0.0, 0.0]
        with pytest.raises(capi.RayzHipError, match=r"status -1"):
            ds.query(torch.tensor(r2, dtype=dt, device="cuda"))
    assert np.array_equal(_run(ds, rays, precision, BVH)["index"], base[BVH]["index"])
    ds.close()


@pytest.mark.parametrize("precision", [F32, F64])
def test_tmin_and_tmax_edges(gpu, oracle, precision):
    s0 = ((0.0, 0.0, -5.0), 1.0, (0.0, 0.0, 0.0))  # roots 4 and 6 along -z from the origin
    sd = _pool([s0, ((0.3, 0.1, -9.0), 0.5, (0.0, 0.0, 0.0))], [((-1.0, -1.0, -7.5), (1.0, -1.0, -7.5), (0.0, 1.0, -7.5))])
    ds = render.DeviceScene(sd)
    ray = np.array([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -1.0, np.inf]])
    # tmin between the two roots: the far root, a back face; tmin = tmax on a root: a hit at that root
    for tmin, tmax, want_i, want_t, front in [(5.0, np.inf, 0, 6.0, 0), (4.0, 4.0, 0, 4.0, 1), (6.0, 6.0, 0, 6.0, 0),
                                              (6.5, 7.5, 2, 7.5, 1), (7.5, 7.5, 2, 7.5, 1), (0.0, 3.0, -1, np.inf, 0)]:
        r = ray.copy()
        r[0, 7] = tmax
        got = _both(ds, r, precision, tmin)
        assert (got["index"][0], float(got["t"][0]), got["front_face"][0]) == (want_i, want_t, front), (tmin, tmax)
    ds.close()
    # a random scene: tmin in {0, 1e-6, 1e-3, 0.5}; a huge finite tmax answers as +inf; tmax < tmin is a miss
    t = SCENES["randomBouncing"]()
    sd = t.scene_desc()
    ds = render.DeviceScene(sd)
    rays = ray_mix(oracle, t, precision, 128, seed=5)
    big = 1e30 if precision == F32 else 1e300
    for tmin in (0.0, 1e-6, 1e-3, 0.5):
        got = _both(ds, rays, precision, tmin)
        s = _exact(sd, rays, got, precision, tmin, what=("tmin", tmin, precision))
        # (at tmin = 0 the secondary rays, which start on a surface, have a root at 0 within the bound of tmin)
        assert s["unambiguous"] >= (0.7 if tmin == 0.0 else 0.8)
        inf_rays = rays[np.isinf(rays[:, 7])]
        huge = inf_rays.copy()
        huge[:, 7] = big
        a, b = _both(ds, inf_rays, precision, tmin), _both(ds, huge, precision, tmin)
        for k in FIELDS:
            assert np.array_equal(a[k], b[k]), (tmin, k)
    below = rays.copy()
    below[:, 7] = np.resize(narrow([-1.0, 0.0, 0.25, float(np.nextafter(narrow(0.5, precision), 0))], precision), len(rays))
    got = _both(ds, below, precision, 0.5)
    assert (got["index"] == -1).all() and (got["material"] == -1).all() and np.isinf(got["t"]).all()
    assert (got["point"] == 0).all() and (got["normal"] == 0).all() and (got["albedo"] == 0).all() and (got["front_face"] == 0).all()
    ds.close()


_SENTINEL = 0x5A


def _outputs(n_alloc, dt):
    kinds = {"index": torch.int32, "material": torch.int32, "front_face": torch.uint8, "hit": torch.uint8}
    width = {"point": 3, "normal": 3, "albedo": 3}
    out = {}
    for k in FIELDS + ("hit",):
        t = torch.empty((n_alloc, width.get(k, 1)), dtype=kinds.get(k, dt), device="cuda")
        t.view(torch.uint8).fill_(_SENTINEL)
        out[k] = t
    return out


def _capi_query(ds, rays_t, n, kind, traversal, precision, outs, given):
    o = capi.QueryOutputs()
    for k in given:
        setattr(o, k, outs[k].data_ptr())
    q = capi.QueryParams(n_rays=n, kind=kind, precision=precision, traversal=traversal, tmin=TMIN)
    torch.cuda.synchronize()
    rc = ds._lib.rayz_hip_scene_query(ds._h, C.byref(q), C.c_void_p(rays_t.data_ptr()), C.byref(o), None)
    assert rc == capi.OK, ds._lib.rayz_hip_last_error()
    assert ds._lib.rayz_hip_query_sync(ds._h, None) == capi.OK
    return {k: v.cpu() for k, v in outs.items()}


def _untouched(t):
    return bool((t.contiguous().view(torch.uint8) == _SENTINEL).all())


@pytest.mark.parametrize("precision", [F32, F64])
def test_output_contract_through_the_c_abi(gpu, oracle, precision):
    """n_rays = 0 touches nothing; for n in {1, 63, 64, 65, 255, 257} nothing past entry n is written by either kernel; outputs
    left NULL are not written; ANY writes `hit` only."""
    t = SCENES["triangleMesh"]()
    sd = t.scene_desc()
    ds = render.DeviceScene(sd)
    dt = torch.float64 if precision == F64 else torch.float32
    rays = ray_mix(oracle, t, precision, 256, seed=9)[:300]
    assert len(rays) >= 257
    rays_t = torch.tensor(rays, dtype=dt, device="cuda")
    ref = _run(ds, rays, precision, BVH)
    n_alloc = len(rays) + 64
    got = _capi_query(ds, rays_t, 0, capi.QUERY_NEAREST, BVH, precision, _outputs(n_alloc, dt), FIELDS + ("hit",))
    assert all(_untouched(v) for v in got.values())
    for n in (1, 63, 64, 65, 255, 257):
        for trav in (LINEAR, BVH):
            got = _capi_query(ds, rays_t, n, capi.QUERY_NEAREST, trav, precision, _outputs(n_alloc, dt), FIELDS + ("hit",))
            for k in FIELDS:
                assert np.array_equal(got[k][:n].numpy().reshape(ref[k][:n].shape), ref[k][:n]), (n, trav, k)
                assert _untouched(got[k][n:]), (n, trav, k, "written past the batch")
            assert np.array_equal(got["hit"][:n, 0].numpy(), (ref["index"][:n] >= 0).astype(np.uint8))
            assert _untouched(got["hit"][n:])
            # a subset: the others stay as they were
            got = _capi_query(ds, rays_t, n, capi.QUERY_NEAREST, trav, precision, _outputs(n_alloc, dt), ("t", "albedo"))
            assert np.array_equal(got["t"][:n, 0].numpy(), ref["t"][:n]) and _untouched(got["t"][n:])
            assert np.array_equal(got["albedo"][:n].numpy(), ref["albedo"][:n])
            for k in ("index", "point", "normal", "front_face", "material", "hit"):
                assert _untouched(got[k]), (n, trav, k)
            # ANY: hit only, whatever else it is given
            got = _capi_query(ds, rays_t, n, capi.QUERY_ANY, trav, precision, _outputs(n_alloc, dt), FIELDS + ("hit",))
            assert np.array_equal(got["hit"][:n, 0].numpy(), (ref["index"][:n] >= 0).astype(np.uint8)) and _untouched(got["hit"][n:])
            for k in FIELDS:
                assert _untouched(got[k]), (n, trav, k, "ANY wrote it")
    ds.close()


def frame_rays(oracle, cam, w, h, precision):
    """getRay(px, py, null) of every pixel, row-major (RAYZ_KAT_GET_RAY, n_u = -1)."""
    py, px = np.divmod(np.arange(w * h), w)
    rec = np.zeros((w * h, capi.KAT_IN_STRIDE))
    for k, f in enumerate([cam.look_from, cam.px_du, cam.px_dv, cam.px_origin, cam.defocus_u, cam.defocus_v]):
        rec[:, 3 * k:3 * k + 3] = list(f)
    rec[:, 18], rec[:, 19], rec[:, 20], rec[:, 21] = cam.defocus, px, py, -1
    kr = oracle.kat_b(capi.KAT_GET_RAY, rec, precision)
    rays = np.zeros((w * h, 8))
    rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7] = kr[:, 0:3], kr[:, 3:6], kr[:, 6], np.inf
    return rays


@pytest.mark.parametrize("scene", ["triangleMesh", "plane_b"])
@pytest.mark.parametrize("precision", [F32, F64])
def test_camera_form_held_to_the_exact_reference(gpu, oracle, scene, precision):
    """The G-buffer of the whole frame (BVH = flat list) against the exact reference on every pixel's ray; three shards are the
    whole frame's rows."""
    t = SCENES[scene]()
    sd, cam = t.scene_desc(), t.camera_desc()
    ds = render.DeviceScene(sd)
    p = t.params()
    p.precision, p.tmin = precision, TMIN
    w, h = p.width, p.height
    whole = {}
    for trav in (BVH, LINEAR):
        p.traversal = trav
        g = ds.gbuffer(cam, p)
        ds.query_sync()
        whole[trav] = {k: getattr(g, k).cpu().numpy() for k in FIELDS}
    for k in FIELDS:
        assert np.array_equal(whole[BVH][k], whole[LINEAR][k]), k
    got = {k: v.reshape((w * h,) + v.shape[2:]) for k, v in whole[BVH].items()}
    s = _exact(sd, frame_rays(oracle, cam, w, h, precision), got, precision, what=("camera", scene, precision))
    assert s["unambiguous"] >= 0.8
    for si in range(3):
        ps = capi.RenderParams.from_buffer_copy(p)
        ps.shard_index, ps.shard_count, ps.tile_rows, ps.traversal = si, 3, 4, BVH
        gs = ds.gbuffer(cam, ps)
        ds.query_sync()
        rows = render.shard_row_indices(h, 4, si, 3)
        for k in FIELDS:
            assert np.array_equal(getattr(gs, k).cpu().numpy(), whole[BVH][k][rows]), (si, k)
    ds.close()
