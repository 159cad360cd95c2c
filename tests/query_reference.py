"""Brute-force `findHit` for the query tests: every primitive of a pool through the oracle's mode-B known-answer pieces
(oracle.binding.kat_b: RAYZ_KAT_SPHERE_HIT / RAYZ_KAT_TRIANGLE_HIT), the nearest root in [tmin, tmax] kept, ties to the
larger hittable index — the order-independent rule every narrow phase of the library applies."""
import numpy as np

from rayz_amd import capi, tracer

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
TMIN = 1e-3


def pool_arrays(scene: capi.SceneDesc):
    """(centers, velocities, radii, sphere materials, triangles (m, 3, 3), triangle materials) of a SceneDesc."""
    ns, nt = scene.n_spheres, scene.n_triangles
    c = np.array([list(scene.spheres[i].center) for i in range(ns)], dtype=np.float64).reshape(-1, 3)
    v = np.array([list(scene.spheres[i].velocity) for i in range(ns)], dtype=np.float64).reshape(-1, 3)
    r = np.array([scene.spheres[i].radius for i in range(ns)], dtype=np.float64)
    sm = np.array([scene.spheres[i].material for i in range(ns)], dtype=np.int64)
    tri = np.array([[list(scene.triangles[i].v0), list(scene.triangles[i].v1), list(scene.triangles[i].v2)] for i in range(nt)],
                   dtype=np.float64).reshape(-1, 3, 3)
    tm = np.array([scene.triangles[i].material for i in range(nt)], dtype=np.int64)
    return c, v, r, sm, tri, tm


def _pairs_near(rays, centers, radii, chunk=1024):
    """(ray, primitive) pairs whose ray LINE passes within 1.01·radius + 1e-3 of the primitive's bounding-sphere centre: a superset
    of every pair with a root (the kat records decide); keeps the oracle's work proportional to the hits, not to n·m."""
    out_r, out_p = [], []
    for a in range(0, len(rays), chunk):
        R = rays[a:a + chunk]
        o, d, tm = R[:, 0:3], R[:, 4:7], R[:, 3]
        ud = d / np.linalg.norm(d, axis=1, keepdims=True)
        cen = centers[0][None, :, :] + centers[1][None, :, :] * tm[:, None, None]
        q = cen - o[:, None, :]
        along = np.einsum("nmk,nk->nm", q, ud)
        dist2 = np.einsum("nmk,nmk->nm", q, q) - along * along
        lim = (1.01 * radii + 1e-3) ** 2
        ri, pi = np.nonzero(dist2 <= lim[None, :])
        out_r.append(ri + a)
        out_p.append(pi)
    return (np.concatenate(out_r) if out_r else np.zeros(0, np.int64)), (np.concatenate(out_p) if out_p else np.zeros(0, np.int64))


def brute_force(oracle, scene: capi.SceneDesc, rays: np.ndarray, tmin: float, precision: int, mode: str = "b"):
    """Per ray: index (-1 on a miss), t (+inf), the known-answer record of the winner (kat_b: point [2..4], normal [5..7],
    front_face [8], passed_filter [9] for spheres) and the second-nearest root's t (+inf).  `rays` (n, 8) float64 holding values
    of the precision.  mode "a": the reference's own functions (kat_a, f64)."""
    rays = np.asarray(rays, dtype=np.float64)
    n = len(rays)
    c, v, r, _, tri, _ = pool_arrays(scene)
    ns = len(c)
    kat = (lambda op, recs: oracle.kat_b(op, recs, precision)) if mode == "b" else oracle.kat_a
    hr, ht, hi, hrec = [], [], [], []
    if ns:
        ri, pi = _pairs_near(rays, (c, v), r)
        for a in range(0, len(ri), 200000):
            rr, pp = ri[a:a + 200000], pi[a:a + 200000]
            recs = np.zeros((len(rr), capi.KAT_IN_STRIDE))
            recs[:, 0:3], recs[:, 3:6], recs[:, 6] = c[pp], v[pp], r[pp]
            recs[:, 7:10], recs[:, 10:13], recs[:, 13] = rays[rr, 0:3], rays[rr, 4:7], rays[rr, 3]
            recs[:, 14], recs[:, 15] = tmin, rays[rr, 7]
            out = kat(capi.KAT_SPHERE_HIT, recs)
            hit = out[:, 0] == 1.0
            hr.append(rr[hit]), ht.append(out[hit, 1]), hi.append(pp[hit]), hrec.append(out[hit])
    if len(tri):
        cen = tri.mean(axis=1)
        rad = np.sqrt(((tri - cen[:, None, :]) ** 2).sum(axis=2)).max(axis=1)
        ri, pi = _pairs_near(rays, (cen, np.zeros_like(cen)), rad)
        for a in range(0, len(ri), 200000):
            rr, pp = ri[a:a + 200000], pi[a:a + 200000]
            recs = np.zeros((len(rr), capi.KAT_IN_STRIDE))
            recs[:, 0:9] = tri[pp].reshape(-1, 9)
            recs[:, 9:12], recs[:, 12:15] = rays[rr, 0:3], rays[rr, 4:7]
            recs[:, 15], recs[:, 16] = tmin, rays[rr, 7]
            out = kat(capi.KAT_TRIANGLE_HIT, recs)
            hit = out[:, 0] == 1.0
            o2 = np.zeros((int(hit.sum()), capi.KAT_OUT_STRIDE))
            o2[:, 0:2] = out[hit, 0:2]
            hr.append(rr[hit]), ht.append(out[hit, 1]), hi.append(pp[hit] + ns), hrec.append(o2)
    best_i = np.full(n, -1, dtype=np.int64)
    best_t = np.full(n, np.inf)
    second_t = np.full(n, np.inf)
    rec_out = np.zeros((n, capi.KAT_OUT_STRIDE))
    if hr:
        R_, T_, I_, X_ = np.concatenate(hr), np.concatenate(ht), np.concatenate(hi), np.concatenate(hrec)
        order = np.lexsort((-I_, T_, R_))  # by ray, then nearest, then the LARGER index first
        R_, T_, I_, X_ = R_[order], T_[order], I_[order], X_[order]
        first = np.ones(len(R_), dtype=bool)
        first[1:] = R_[1:] != R_[:-1]
        best_i[R_[first]], best_t[R_[first]], rec_out[R_[first]] = I_[first], T_[first], X_[first]
        nxt = np.zeros(len(R_), dtype=bool)
        nxt[1:] = first[:-1] & ~first[1:]
        second_t[R_[nxt]] = T_[nxt]
    return best_i, best_t, rec_out, second_t


def albedo_of(oracle, scene: capi.SceneDesc, material: int, point, precision: int):
    """texture_value at `point` walked on the host: solids narrowed to the precision, checkers decided by RAYZ_KAT_CHECKER."""
    m = scene.materials[material]
    if m.kind == capi.MAT_DIELECTRIC:
        return np.ones(3)
    idx = m.texture
    for _ in range(8):
        t = scene.textures[idx]
        if t.kind == capi.TEX_SOLID:
            col = np.array(list(t.color))
            return col.astype(np.float32).astype(np.float64) if precision == capi.PRECISION_F32 else col
        rec = np.zeros((1, capi.KAT_IN_STRIDE))
        rec[0, 0:3], rec[0, 3] = point, t.scale
        parity = oracle.kat_b(capi.KAT_CHECKER, rec, precision)[0, 0]
        idx = t.even if parity == 0 else t.odd
    return np.zeros(3)


# ---- scenes and ray mixes of the query tests (no GPU needed: the oracle makes the rays) ----------------------------------
def plane_scene(seed):
    """(as tests/test_fuzz_gpu.py builds them) plane runs: 1 to 6 heights, 40 / 63 / 64 / 65 / 100 / 257 spheres each, static or
    y-moving per height, among loose, generally moving spheres and a ground sphere; random materials."""
    rng = np.random.default_rng(seed)
    n_h = int(rng.integers(1, 7))
    hs = [float(rng.choice([0.0, -0.0, float(rng.uniform(-2.5, -0.1)), float(rng.uniform(0.1, 3.0))])) for _ in range(n_h)]
    level = rng.random() < 0.4
    if level:
        h = hs[int(rng.integers(0, n_h))]
        look_from, look_at = np.array([-14.0, h, float(rng.uniform(-1, 1))]), np.array([10.0, h, float(rng.uniform(-1, 1))])
    else:
        look_from, look_at = rng.uniform(-8, 8, 3) + np.array([0, 6.0, 0]), rng.uniform(-1, 1, 3)
    t = tracer.Tracer.init(int(rng.integers(24, 48)), float(rng.uniform(25, 60)), float(rng.uniform(4, 12)),
                           float(rng.choice([0.0, 0.0, 1.0])), look_from, look_at, (0, 1, 0), seed=seed)
    P = t.pool
    tex = [P.add_solid_texture(rng.uniform(0.05, 0.95, 3)) for _ in range(3)]
    tex.append(P.add_checker_texture(float(rng.uniform(0.2, 1.0)), tex[0], tex[1]))
    mats = [P.add_diffuse(int(rng.choice(tex)), int(rng.integers(0, 3))) for _ in range(3)]
    mats += [P.add_metallic(int(rng.choice(tex)), float(rng.choice([0.0, rng.uniform(0, 1)]))), P.add_dielectric(1.5)]
    rows = [((0.0, -1004.0, 0.0), 1000.0, (0.0, 0.0, 0.0))]
    for h in hs:
        movy = rng.random() < 0.5
        spread = float(rng.uniform(3, 9))
        for _ in range(int(rng.choice([40, 63, 64, 65, 100, 257]))):
            v = (0.0, float(rng.uniform(0.05, 0.6) * rng.choice([-1, 1])), 0.0) if movy else (0.0, 0.0, 0.0)
            rows.append(((float(rng.uniform(-spread, spread)), h, float(rng.uniform(-spread, spread))), float(rng.uniform(0.1, 0.6)), v))
    for _ in range(int(rng.integers(0, 20))):
        cls = rng.integers(0, 3)
        v = (0, 0, 0) if cls == 0 else ((0, float(rng.uniform(-1, 1)), 0) if cls == 1 else tuple(rng.uniform(-1, 1, 3)))
        rows.append((tuple(rng.uniform((-6, -2.5, -6), (6, 3, 6))), float(rng.uniform(0.2, 0.9)), v))
    for k in rng.permutation(len(rows)):
        c, r, v = rows[k]
        P.add_sphere(c, r, int(rng.choice(mats)), velocity=v)
    t.samples_per_px = int(rng.integers(1, 8))
    t.max_bounces = int(rng.integers(2, 12))
    t.set_gpu(render_seed=int(rng.integers(0, 2 ** 62)), chunk_spp=int(rng.choice([0, 1, 16])))
    return t


def narrow(a, precision):
    return np.asarray(a, dtype=np.float64).astype(np.float32).astype(np.float64) if precision == F32 else np.asarray(a, np.float64)


def camera_rays(oracle, cam: capi.CameraDesc, w, h, precision, n, rng):
    """getRay(px, py, null) through the oracle's RAYZ_KAT_GET_RAY with n_u = -1, for n random pixels."""
    px, py = rng.integers(0, w, n), rng.integers(0, h, n)
    rec = np.zeros((n, capi.KAT_IN_STRIDE))
    fields = [cam.look_from, cam.px_du, cam.px_dv, cam.px_origin, cam.defocus_u, cam.defocus_v]
    for k, f in enumerate(fields):
        rec[:, 3 * k:3 * k + 3] = list(f)
    rec[:, 18], rec[:, 19], rec[:, 20], rec[:, 21] = cam.defocus, px, py, -1
    out = oracle.kat_b(capi.KAT_GET_RAY, rec, precision)
    rays = np.zeros((n, 8))
    rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7] = out[:, 0:3], out[:, 3:6], out[:, 6], np.inf
    return rays, px, py


def ray_mix(oracle, t: tracer.Tracer, precision, n, seed):
    """Camera rays, secondary rays from their first hits, rays grazing sphere silhouettes, rays starting inside spheres, finite
    tmax on and between roots, times 0, 0.5 and 1."""
    rng = np.random.default_rng(seed)
    sd, cam = t.scene_desc(), t.camera_desc()
    info = t.params()
    cr, _, _ = camera_rays(oracle, cam, info.width, info.height, precision, n, rng)
    cr[:, 3] = rng.choice([0.0, 0.5, 1.0], n)
    idx, tt, rec, _ = brute_force(oracle, sd, cr, TMIN, precision)
    c, v, r, _, tri, _ = pool_arrays(sd)
    parts = [cr]
    # secondary: from first-hit points along a random direction
    hit = np.nonzero(idx >= 0)[0]
    if len(hit):
        o = cr[hit, 0:3] + cr[hit, 4:7] * tt[hit, None]
        dirs = rng.normal(size=(len(hit), 3))
        sec = np.concatenate([o, rng.choice([0.0, 0.5, 1.0], (len(hit), 1)), dirs, np.full((len(hit), 1), np.inf)], axis=1)
        parts.append(sec)
        # finite tmax exactly on the first root, and just before it (a miss unless something nearer)
        on = cr[hit].copy()
        on[:, 7] = tt[hit]
        before = cr[hit].copy()
        before[:, 7] = tt[hit] * 0.999
        parts += [on, before]
        # .. and between the near and the far root of the winning sphere
        sw = hit[idx[hit] < len(c)] if len(c) else hit[:0]
        if len(sw):
            k = idx[sw]
            q = c[k] + v[k] * cr[sw, 3:4] - cr[sw, 0:3]
            d = cr[sw, 4:7]
            a2, hb = (d * d).sum(axis=1), (d * q).sum(axis=1)
            far = (hb + np.sqrt(np.maximum(hb * hb - a2 * ((q * q).sum(axis=1) - r[k] ** 2), 0.0))) / a2
            mid = cr[sw].copy()
            mid[:, 7] = 0.5 * (tt[sw] + far)
            parts.append(mid)
    if len(c):
        m = n // 2
        k = rng.integers(0, len(c), m)
        tm = rng.choice([0.0, 0.5, 1.0], m)
        cen = c[k] + v[k] * tm[:, None]
        # grazing: aimed at a point on the silhouette seen from the camera, scaled by 1 ± 1e-6
        o = np.tile(np.array(list(cam.look_from)), (m, 1)) + rng.normal(scale=0.5, size=(m, 3))
        to = cen - o
        perp = np.cross(to, rng.normal(size=(m, 3)))
        perp /= np.linalg.norm(perp, axis=1, keepdims=True)
        target = cen + perp * (r[k] * (1 + rng.choice([-1e-6, 0.0, 1e-6], m)))[:, None]
        parts.append(np.concatenate([o, tm[:, None], target - o, np.full((m, 1), np.inf)], axis=1))
        # inside: origin at half the radius from the centre
        u = rng.normal(size=(m, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        parts.append(np.concatenate([cen + u * (0.5 * r[k])[:, None], tm[:, None], rng.normal(size=(m, 3)), np.full((m, 1), np.inf)], axis=1))
    rays = narrow(np.concatenate(parts), precision)
    bad = ~np.isfinite(rays[:, 0:7]).all(axis=1) | (np.abs(rays[:, 4:7]).sum(axis=1) == 0)
    return rays[~bad]


SCENES = {
    "threeSpheres": lambda: tracer.threeSpheres(48, seed=3),
    "randomBouncing": lambda: tracer.randomBouncing(48, -3, 3, seed=5),
    "triangleMesh": lambda: tracer.triangleMesh(48, 10, seed=1),
    "plane_a": lambda: plane_scene(11),
    "plane_b": lambda: plane_scene(23),
}
