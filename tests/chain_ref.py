"""The specular-chain G-buffer's contract restated ONCE, as a composition over a backend: `chain()` below is the
whole rule; a backend supplies the four pieces it composes — `get_ray` (getRay(px, py, null)), `find_hit` (the NEAREST `findHit`
record), `scatter` (Material.scatter's direction on a draw list) and `albedo` (texture_value, (1, 1, 1) for glass).

OracleBackend takes them from the CPU oracle's mode-B known-answer pieces (query_reference.brute_force / albedo_of, oracle.kat_b);
DeviceBackend from the library's public ray queries and known-answer entry (DeviceScene.query, render.kat).  Neither runs the
chain kernels.  All arrays are float64 holding values of the precision."""
import math
from fractions import Fraction

import numpy as np

import query_reference as qr
from rayz_amd import capi

KEY_MUL = 0x9E3779B1
INF = float("inf")


def _rt(precision):
    return np.float32 if precision == capi.PRECISION_F32 else np.float64


def chain(backend, cam: capi.CameraDesc, px, py, tmin: float, max_depth: int, max_fuzz: float):
    """The chain of every pixel (px[k], py[k]).  Returns a dict of arrays: the LAST segment's record (index, t, point, normal,
    front_face, material, albedo = tint x albedo_last), key (uint32), depth, first_index, segments = depth + 1; and, for the tests'
    bookkeeping only, `dir` (the last segment's direction) and the flags `tir` (some followed hit was totally reflected),
    `fuzz_stop` (ended on a metal refused by max_fuzz) and `specular_end` (ended at max_depth on a record that would be followed)."""
    rt = _rt(backend.precision)
    mul = lambda a, b: (np.asarray(a, rt) * np.asarray(b, rt)).astype(np.float64)  # noqa: E731  (one rounding in R)
    n = len(px)
    out = dict(index=np.full(n, -1, np.int64), t=np.full(n, INF), point=np.zeros((n, 3)), normal=np.zeros((n, 3)),
               front_face=np.zeros(n, np.int64), material=np.full(n, -1, np.int64), albedo=np.zeros((n, 3)),
               key=np.zeros(n, np.uint32), depth=np.zeros(n, np.int64), first_index=np.full(n, -1, np.int64), dir=np.zeros((n, 3)),
               tir=np.zeros(n, bool), fuzz_stop=np.zeros(n, bool), specular_end=np.zeros(n, bool))
    rays = backend.get_ray(cam, px, py)  # segment 0: time 0, tmax +inf
    tint = np.ones((n, 3))
    key = np.zeros(n, np.uint64)
    active = np.arange(n)
    for s in range(max_depth + 1):
        hit = backend.find_hit(rays, tmin)  # the NEAREST query of segment s
        m = len(active)
        idx = hit["index"]
        alb = backend.albedo(hit)  # (0, 0, 0) on a miss
        if s == 0:
            out["first_index"][active] = idx
        kind, param = backend.material(hit["material"])  # (-1, 0) on a miss; the parameter narrowed to the precision
        diel, metal = kind == capi.MAT_DIELECTRIC, kind == capi.MAT_METALLIC
        specular = (idx >= 0) & (diel | (metal & ~(param > max_fuzz)))
        follow = specular & (s < max_depth)
        nd = np.zeros((m, 3))
        f = np.nonzero(follow)[0]
        if len(f):  # the metal's fuzz taken as 0, every uniform 1.0
            ok, nd[f] = backend.scatter(kind[f], np.where(metal[f], 0.0, param[f]), rays[f, 4:7], hit["point"][f], hit["normal"][f],
                                        hit["front_face"][f])
            follow[f] = ok  # (a metal may absorb)
        end = ~follow
        e = active[end]
        for k in ("index", "t", "point", "normal", "front_face", "material"):
            out[k][e] = hit[k][end]
        out["albedo"][e] = mul(tint[end], alb[end])
        out["key"][e] = key[end].astype(np.uint32)
        out["dir"][e] = rays[end, 4:7]
        out["fuzz_stop"][e] = (idx >= 0)[end] & metal[end] & (param > max_fuzz)[end]
        out["specular_end"][e] = specular[end] & (s == max_depth)
        # the followed hits
        g = np.nonzero(follow)[0]
        a = active[g]
        out["depth"][a] += 1
        key = (key[g] * np.uint64(KEY_MUL) + (idx[g] + 1).astype(np.uint64)) & np.uint64(0xFFFFFFFF)
        tint = mul(tint[g], alb[g])
        out["tir"][a] |= diel[g] & _tir(rays[g, 4:7], hit["normal"][g], hit["front_face"][g], param[g])
        nxt = np.zeros((len(g), 8))
        nxt[:, 0:3], nxt[:, 4:7], nxt[:, 7] = hit["point"][g], nd[g], INF
        rays, active = nxt, a
        if not len(active):
            break
    out["segments"] = out["depth"] + 1
    return out


def _tir(d, nrm, front, ior):
    """eta·sin > 1, in float64 (bookkeeping: which pixels saw a total internal reflection)."""
    ud = d / np.linalg.norm(d, axis=1, keepdims=True)
    cos = -(ud * nrm).sum(axis=1)
    eta = np.where(front != 0, 1.0 / np.where(ior == 0, 1.0, ior), ior)
    return eta * np.sqrt(np.maximum(1.0 - cos * cos, 0.0)) > 1.0


# ---- the pieces both backends build their records from ---------------------------------------------------------------------
def _get_ray_records(cam, px, py):
    rec = np.zeros((len(px), capi.KAT_IN_STRIDE))
    for k, f in enumerate([cam.look_from, cam.px_du, cam.px_dv, cam.px_origin, cam.defocus_u, cam.defocus_v]):
        rec[:, 3 * k:3 * k + 3] = list(f)
    rec[:, 18], rec[:, 19], rec[:, 20], rec[:, 21] = cam.defocus, px, py, -1  # n_u = -1: getRay(px, py, null)
    return rec


def _rays_of(out):
    rays = np.zeros((len(out), 8))
    rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7] = out[:, 0:3], out[:, 3:6], out[:, 6], INF
    return rays


def _scatter_records(kind, param, d, point, normal, front):
    rec = np.zeros((len(kind), capi.KAT_IN_STRIDE))
    rec[:, 0], rec[:, 1], rec[:, 2] = kind, 0, param
    rec[:, 3:6], rec[:, 6:9], rec[:, 9:12], rec[:, 12:15], rec[:, 15] = point, d, point, normal, front
    rec[:, 16], rec[:, 17] = 1, 1.0  # the draw list [1.0]
    return rec


class _Backend:
    def __init__(self, sd: capi.SceneDesc, precision: int):
        self.sd, self.precision = sd, precision
        self._kind = np.array([sd.materials[i].kind for i in range(sd.n_materials)], np.int64)
        self._param = qr.narrow([sd.materials[i].param for i in range(sd.n_materials)], precision)
        self._hits = {}

    def material(self, mat):
        ok = mat >= 0
        safe = np.where(ok, mat, 0)
        return np.where(ok, self._kind[safe], -1), np.where(ok, self._param[safe], 0.0)

    def find_hit(self, rays, tmin):
        """The records of `rays`, each ray computed once (a chain of any max_depth starts with the rays of a shorter one)."""
        keys = [(r.tobytes(), tmin) for r in rays]
        new = [i for i, k in enumerate(keys) if k not in self._hits]
        if new:
            got = self._find_hit(rays[new], tmin)
            for j, i in enumerate(new):
                self._hits[keys[i]] = {k: v[j] for k, v in got.items()}
        rows = [self._hits[k] for k in keys]
        return {k: np.stack([r[k] for r in rows]) for k in ("index", "t", "point", "normal", "front_face", "material", "albedo")}

    def albedo(self, hit):
        return hit["albedo"]


# ---- exact arithmetic for the one record the oracle's known-answer pieces do not hold: a triangle's point and normal ---------
def _round(fr: Fraction, rt):
    """fr rounded to nearest-even in rt."""
    if rt is np.float64:
        return float(fr)  # (int / int division of a Fraction is correctly rounded)
    x = np.float32(float(fr))
    cands = sorted({float(np.nextafter(x, np.float32(-INF))), float(x), float(np.nextafter(x, np.float32(INF)))})
    best = min(cands, key=lambda c: (abs(Fraction(c) - fr), int(np.float32(c).view(np.uint32)) & 1))
    return best


def _fma(a, b, c, rt):
    return _round(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)), rt)


def _tri_record(v0, v1, v2, o, d, t, rt):
    """pt = fm(d, t, o); n = unit(cross3(e1, e2)) with e = (R)(v - v0), flipped to face the ray — the arithmetic of the device's
    hit record (device_math.hpp: cross3, dot3, unit; shade.hpp: face_forward), one rounding per operation, FMAs exact."""
    r = lambda x: float(rt(x))  # noqa: E731
    e1, e2 = [r(v1[k] - v0[k]) for k in range(3)], [r(v2[k] - v0[k]) for k in range(3)]
    pt = [_fma(d[k], t, o[k], rt) for k in range(3)]
    cr = [_fma(e1[1], e2[2], -r(rt(e1[2]) * rt(e2[1])), rt), _fma(e1[2], e2[0], -r(rt(e1[0]) * rt(e2[2])), rt),
          _fma(e1[0], e2[1], -r(rt(e1[1]) * rt(e2[0])), rt)]
    dot = lambda a, b: _fma(a[2], b[2], _fma(a[1], b[1], r(rt(a[0]) * rt(b[0])), rt), rt)  # noqa: E731
    inv = r(rt(1) / rt(math.sqrt(dot(cr, cr)) if rt is np.float64 else np.sqrt(rt(dot(cr, cr)))))
    nrm = [r(rt(c) * rt(inv)) for c in cr]
    front = dot(nrm, d) < 0
    if not front:
        nrm = [-c for c in nrm]
    return pt, nrm, 1 if front else 0


class OracleBackend(_Backend):
    """The CPU oracle's mode-B pieces."""

    def __init__(self, oracle, sd, precision):
        super().__init__(sd, precision)
        self.oracle = oracle
        _, _, _, self._sm, self._tri, self._tm = qr.pool_arrays(sd)

    def get_ray(self, cam, px, py):
        return _rays_of(self.oracle.kat_b(capi.KAT_GET_RAY, _get_ray_records(cam, px, py), self.precision))

    def _find_hit(self, rays, tmin):
        rt = _rt(self.precision)
        idx, t, rec, _ = qr.brute_force(self.oracle, self.sd, rays, tmin, self.precision)
        n, ns = len(rays), len(self._sm)
        out = dict(index=idx, t=t, point=np.zeros((n, 3)), normal=np.zeros((n, 3)), front_face=np.zeros(n, np.int64),
                   material=np.full(n, -1, np.int64), albedo=np.zeros((n, 3)))
        sph = (idx >= 0) & (idx < ns)
        out["point"][sph], out["normal"][sph], out["front_face"][sph] = rec[sph, 2:5], rec[sph, 5:8], rec[sph, 8]
        out["material"][sph] = self._sm[idx[sph]]
        for i in np.nonzero(idx >= ns)[0]:
            v = self._tri[idx[i] - ns]
            out["point"][i], out["normal"][i], out["front_face"][i] = _tri_record(v[0], v[1], v[2], rays[i, 0:3], rays[i, 4:7], t[i], rt)
            out["material"][i] = self._tm[idx[i] - ns]
        for i in np.nonzero(idx >= 0)[0]:
            out["albedo"][i] = qr.albedo_of(self.oracle, self.sd, int(out["material"][i]), out["point"][i], self.precision)
        return out

    def scatter(self, kind, param, d, point, normal, front):
        out = self.oracle.kat_b(capi.KAT_SCATTER, _scatter_records(kind, param, d, point, normal, front), self.precision)
        return out[:, 0] == 1.0, out[:, 1:4]


class DeviceBackend(_Backend):
    """The library's public queries and known-answer entry on a DeviceScene (`render`: rayz_amd.render, initialised)."""

    def __init__(self, render, scene, sd, precision, traversal=capi.TRAVERSAL_LINEAR):
        super().__init__(sd, precision)
        self.render, self.scene, self.traversal = render, scene, traversal

    def get_ray(self, cam, px, py):
        return _rays_of(self.render.kat(capi.KAT_GET_RAY, _get_ray_records(cam, px, py), self.precision))

    def _find_hit(self, rays, tmin):
        import torch

        dt = torch.float32 if self.precision == capi.PRECISION_F32 else torch.float64
        r = self.scene.query(torch.tensor(rays, dtype=dt, device=torch.device("cuda", self.scene.device)), tmin=tmin,
                             traversal=self.traversal)
        self.scene.query_sync()
        return {k: getattr(r, k).cpu().numpy().astype(np.int64 if k in ("index", "front_face", "material") else np.float64)
                for k in ("index", "t", "point", "normal", "front_face", "material", "albedo")}

    def scatter(self, kind, param, d, point, normal, front):
        out = self.render.kat(capi.KAT_SCATTER, _scatter_records(kind, param, d, point, normal, front), self.precision)
        return out[:, 0] == 1.0, out[:, 1:4]
