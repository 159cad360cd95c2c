"""Scenes that hand the BVH kernels every layout their tree can take (rayz_amd/csrc/bvh_build.hpp, upload_bvh_body): several
oversized hittables kept out of the tree — spheres, moving spheres and triangles, packed two to a descriptor —, the cap of eight,
the stop at kMinTree hittables, and a tree whose depth sits at the surface-area split's budget.  Every scene goes through
tracer.Tracer.init and its pool; `layout()` runs the library's own builder on it (tests/bvh_layout_mirror.cpp) and `check_layout()`
asserts that the scene forms the layout it was built for, so a change of the builder cannot quietly turn these scenes into ordinary
ones.  `query_rays()` makes each scene's ray set for the query kernels.

The room: a cluster of small spheres over x, z in [-4, 4], bounded by huge spheres whose surfaces pass at y = 0 (floor), x = -8,
z = -6, x = 5, y = 4 (ceiling) and z = 10; the camera stands inside it and looks at the cluster.  The ceiling and the wall behind
the camera are glass, and so are the walls left and right: the sky is the only light, and a closed room of opaque walls renders
black."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np

from query_reference import TMIN, brute_force, narrow, pool_arrays, ray_mix
from rayz_amd import capi, tracer

HERE = os.path.dirname(os.path.abspath(__file__))

WALLS = [((0.0, -1000.0, 0.0), 1000.0), ((-808.0, 0.0, 0.0), 800.0), ((0.0, 0.0, -606.0), 600.0), ((505.0, 0.0, 0.0), 500.0),
         ((0.0, 404.0, 0.0), 400.0), ((0.0, 0.0, 310.0), 300.0)]
ROOM_LO, ROOM_HI = np.array([-7.0, 0.3, -5.0]), np.array([4.8, 3.6, 9.0])  # well inside all six walls
STILL = (0.0, 0.0, 0.0)

NAMES = [f"walls{k}" for k in range(7)] + ["mixed5", "nine", "pool30", "pool31", "pool32", "pool33", "line600"]
QUERY_NAMES = ["walls2", "walls3", "mixed5", "nine", "pool31", "line600"]
# what is kept out of the tree, in peel order: s = sphere, m = moving sphere, t = triangle
PEELED = {**{f"walls{k}": "s" * k for k in range(7)}, "mixed5": "sttmt", "nine": "sssssstt", "pool30": "s", "pool31": "ss",
          "pool32": "sss", "pool33": "sss", "line600": ""}


def _materials(P):
    tex = [P.add_solid_texture(c) for c in ((0.8, 0.3, 0.3), (0.3, 0.7, 0.4), (0.9, 0.9, 0.9), (0.2, 0.3, 0.8))]
    tex.append(P.add_checker_texture(0.8, tex[1], tex[2]))
    return [P.add_diffuse(tex[0]), P.add_diffuse(tex[4]), P.add_metallic(tex[2], 0.0), P.add_metallic(tex[3], 0.3),
            P.add_dielectric(1.5), P.add_diffuse(tex[1], 1)]


def _room_tracer(seed):
    return tracer.Tracer.init(64, 60.0, 8.0, 0.0, (1.5, 2.0, 8.5), (0.0, 1.2, 0.0), (0, 1, 0), seed=seed)


def _cluster(n, seed):
    """(centre, radius, velocity, material slot) of n small spheres; every fifth moves."""
    rng = np.random.default_rng(seed)
    rows = []
    for i in range(n):
        c = (float(rng.uniform(-4, 4)), float(rng.uniform(0.4, 2.4)), float(rng.uniform(-4, 4)))
        v = tuple(rng.uniform(-0.3, 0.3, 3)) if i % 5 == 4 else STILL
        rows.append(("s", c, float(rng.uniform(0.2, 0.4)), v, int(rng.integers(0, 6))))
    return rows


def _walls(k):
    # floor: checker; left: glass; far: mirror; right, ceiling, behind the camera: glass
    return [("s", c, r, STILL, (1, 4, 2, 4, 4, 4)[i]) for i, (c, r) in enumerate(WALLS[:k])]


def _rows(name):
    """The pool in order: the outliers sit in the middle of the cluster, so that pool order, peel order and leaf order all differ."""
    if name.startswith("walls"):
        cl, out = _cluster(60, 7), _walls(int(name[5:]))
    elif name == "mixed5":
        cl = _cluster(60, 11)
        out = [("t", (-20.0, 0.03, -20.0), (20.0, 0.03, -20.0), (0.0, 0.03, 20.0), 3),  # extent 40
               ("s", (0.0, 50.0, 0.0), 30.0, (0.0, 25.0, 0.0), 2),  # moving: box 60 x 85 x 60
               ("s", WALLS[0][0], WALLS[0][1], STILL, 1),
               ("t", (-100.0, -5.0, -40.0), (100.0, -5.0, -40.0), (0.0, 120.0, -45.0), 0),  # tall: extent 200
               ("t", (-300.0, 0.02, -300.0), (300.0, 0.02, -300.0), (0.0, 0.02, 300.0), 5)]  # floor: extent 600
    elif name == "nine":
        cl = _cluster(60, 13)
        out = _walls(6) + [("s", (0.0, 60.0, 0.0), 40.0, (0.0, 30.0, 0.0), 3),  # box 80 x 110 x 80: the ninth, stays in the tree
                           ("t", (-90.0, 0.05, -90.0), (90.0, 0.05, -90.0), (90.0, 0.05, 90.0), 1),
                           ("t", (-90.0, 0.05, -90.0), (90.0, 0.05, 90.0), (-90.0, 0.05, 90.0), 5)]
    elif name.startswith("pool"):
        cl, out = _cluster(int(name[4:]), 17), _walls(3)
    else:
        raise KeyError(name)
    half = len(cl) // 2
    return cl[:half] + out + cl[half:]


def make(name):
    """A fresh tracer of the scene (64x36, 8 spp, 12 bounces)."""
    if name == "line600":  # seen along the line, from over its large end
        t = tracer.Tracer.init(64, 50.0, 100.0, 0.0, (1200.0, 6.0, 8.0), (2354.0, 0.0, 0.0), (0, 1, 0), seed=3)
        mats = _materials(t.pool)
        rng = np.random.default_rng(19)
        x, r = 0.0, 0.01
        for i in range(600):
            t.pool.add_sphere((x, 0.0, 0.0), r, mats[i % 6])
            x += 2.2 * r + float(rng.uniform(0, 6e-3))
            r *= 1.012
    else:
        t = _room_tracer(5)
        mats = _materials(t.pool)
        for row in _rows(name):
            if row[0] == "s":
                t.pool.add_sphere(row[1], row[2], mats[row[4]], velocity=row[3])
            else:
                t.pool.add_triangle(row[1], row[2], row[3], mats[row[4]])
    t.samples_per_px, t.max_bounces = 8, 12
    t.set_gpu(render_seed=21)
    return t


# ---- the layout, by the library's own builder -------------------------------------------------------------------------------------
def mirror_exe(directory):
    """tests/bvh_layout_mirror.cpp compiled into `directory` (the tests' module fixtures call it once each)."""
    gxx = shutil.which("g++")
    assert gxx, "the layout mirror needs g++"
    exe = os.path.join(directory, "bvh_layout_mirror")
    subprocess.run([gxx, "-std=c++17", "-O2", "-o", exe, os.path.join(HERE, "bvh_layout_mirror.cpp")], check=True, capture_output=True,
                   timeout=300)
    return exe


def layout(exe, sd, path):
    """{(peel, sah): the mirror's record} for a SceneDesc."""
    with open(path, "wb") as f:
        f.write(np.array([sd.n_spheres, sd.n_triangles], dtype=np.uint64).tobytes())
        f.write(C.string_at(sd.spheres, sd.n_spheres * C.sizeof(capi.Sphere)))
        if sd.n_triangles:
            f.write(C.string_at(sd.triangles, sd.n_triangles * C.sizeof(capi.Triangle)))
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return {(e["peel"], e["sah"]): e for e in json.loads(r.stdout)}


def kind_of(sd, i):
    if i >= sd.n_spheres:
        return "t"
    return "m" if any(sd.spheres[i].velocity) else "s"


def _extent(sd, i):
    c, v, r, _, tri, _ = pool_arrays(sd)
    if i >= sd.n_spheres:
        return float((tri[i - sd.n_spheres].max(axis=0) - tri[i - sd.n_spheres].min(axis=0)).max()) + 2e-4
    return float((2 * r[i] + np.abs(v[i])).max())


def check_layout(name, sd, lay):
    """The layout `name` was built for, asserted on the mirror's records.  Returns the peeled pool indices."""
    n = sd.n_spheres + sd.n_triangles
    want = PEELED[name]
    for sah in (0, 1):
        whole, e = lay[(0, sah)], lay[(1, sah)]
        assert whole["big"] == [] and whole["descriptors"] == [] and whole["in_tree"] == n  # PEEL = 0: everything in the tree
        big = e["big"]
        assert "".join(kind_of(sd, i) for i in big) == want, (name, big)
        assert e["in_tree"] == n - len(big) and e["max_big"] == 8 and e["min_tree"] == 32
        ext = [_extent(sd, i) for i in big]
        assert ext == sorted(ext, reverse=True) and all(x > 20 for x in ext)  # largest first, and outliers indeed
        # the descriptors: two entries each in peel order, slots after the tree's, a type bit per entry
        assert len(e["descriptors"]) == (len(big) + 1) // 2
        for k, d in enumerate(e["descriptors"]):
            pair = big[2 * k:2 * k + 2]
            assert d["first"] == e["in_tree"] + 2 * k and d["count"] == len(pair)
            assert d["triangle"][:len(pair)] == [int(i >= sd.n_spheres) for i in pair] and (len(pair) == 2 or d["triangle"][1] == 0)
            assert d["word"] == (d["first"] << 4) | (d["triangle"][1] << 3) | (d["triangle"][0] << 2) | d["count"]
        assert e["nodes"] == 2 * (e["nodes"] - e["inner"]) - 1
    e = lay[(1, 1)]  # the tree the device walks by default
    assert e["depth"] <= e["budget"]
    big = e["big"]
    others = [i for i in range(n) if i not in big]
    if name.startswith("walls"):
        k = int(name[5:])
        assert len(big) == k and big == sorted(big)  # exactly the first k walls, in pool order
        assert [tuple(sd.spheres[i].center) for i in big] == [w[0] for w in WALLS[:k]]
        assert [d["count"] for d in e["descriptors"]] == [2] * (k // 2) + [1] * (k % 2)
    elif name == "mixed5":
        assert [(d["count"], d["triangle"]) for d in e["descriptors"]] == [(2, [0, 1]), (2, [1, 0]), (1, [1, 0])]
    elif name == "nine":
        assert len(big) == 8 and len(e["descriptors"]) == 4
        left = [i for i in others if _extent(sd, i) > 20]  # the ninth outlier: in the tree only because the cap was reached
        assert len(left) == 1 and kind_of(sd, left[0]) == "m" and _extent(sd, left[0]) < min(_extent(sd, i) for i in big)
    elif name.startswith("pool"):
        left = [i for i in others if _extent(sd, i) > 20]
        assert len(big) + len(left) == 3
        assert e["in_tree"] == max(32, n - 3)  # peeling stopped when 32 were left, or when the outliers ran out
        assert (len(left) > 0) == (name in ("pool30", "pool31"))
    else:
        assert name == "line600" and big == [] and n == 600
        assert e["depth"] == e["budget"] == 14 and lay[(0, 0)]["depth"] == 10  # the SAH tree at its depth budget; median tree
    return big


# ---- rays for the query kernels ---------------------------------------------------------------------------------------------------
def _outlier_scene(sd, big):
    """A SceneDesc of the peeled hittables alone (one material): what a ray meets among them, by brute force."""
    from test_query_cpu import _pool

    c, v, r, _, tri, _ = pool_arrays(sd)
    ns = sd.n_spheres
    return _pool([(tuple(c[i]), float(r[i]), tuple(v[i])) for i in big if i < ns],
                 [tuple(map(tuple, tri[i - ns])) for i in big if i >= ns])


def _rays(o, time, d, tmax=np.inf):
    n = len(o)
    return np.concatenate([o, np.broadcast_to(np.asarray(time, dtype=np.float64).reshape(-1, 1), (n, 1)), d,
                           np.broadcast_to(np.asarray(tmax, dtype=np.float64).reshape(-1, 1), (n, 1))], axis=1)


def aimed_rays(sd, big, rng, per=12):
    """Rays at every peeled hittable, from inside the room and (the same line, reversed) from beyond it; times 0, 0.5, 1."""
    c, v, r, _, tri, _ = pool_arrays(sd)
    ns = sd.n_spheres
    mid = np.array([0.0, 1.5, 0.0])
    out = []
    for i in big:
        o = rng.uniform(ROOM_LO, ROOM_HI, (per, 3))
        time = rng.choice([0.0, 0.5, 1.0], per)
        if i < ns:
            cen = c[i] + v[i] * time[:, None]
            u = mid + rng.normal(scale=2.0, size=(per, 3)) - cen
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            near = cen + u * r[i]  # on the surface, where it passes the room
            w = rng.normal(size=(per, 3))
            inside = cen + w / np.linalg.norm(w, axis=1, keepdims=True) * (r[i] * rng.uniform(0, 0.9, (per, 1)))
            target = np.where((np.arange(per) % 2 == 0)[:, None], near, inside)
            reach = np.linalg.norm(target - o, axis=1) + 2.5 * r[i]
        else:
            b = rng.dirichlet([1, 1, 1], per)
            target = b @ tri[i - ns]
            reach = np.linalg.norm(target - o, axis=1) + 50.0
        d = target - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        out.append(_rays(o, time, d * rng.uniform(0.5, 2.0, (per, 1))))
        far = o + d * reach[:, None]  # beyond the hittable: the same line back hits it from its other side
        out.append(_rays(far, time, -d * rng.uniform(0.5, 2.0, (per, 1))))
    return np.concatenate(out) if out else np.zeros((0, 8))


def tmax_rays(oracle, sd, big, rays, precision):
    """The aimed rays again with a finite tmax just in front of, on and just behind the nearest root among the peeled hittables."""
    rays = narrow(rays, precision)
    _, t, _, _ = brute_force(oracle, _outlier_scene(sd, big), rays, TMIN, precision)
    hit = np.isfinite(t)
    out = []
    for f in (0.999, 1.0, 1.001):
        pick = np.flatnonzero(hit)[::2 if f == 1.0 else 1]  # (a tmax on the root is ambiguous by construction: half as many)
        q = rays[pick].copy()
        q[:, 7] = narrow(t[pick] * f, precision)
        out.append(q)
    return np.concatenate(out)


def only_triangle_rays(name, sd, big, rng, n=128):
    """Two waves whose only hit in range is one oversized triangle: a short ray straight through it, where nothing else is near.
    Returns (rays, the triangle's pool index)."""
    _, _, _, _, tri, _ = pool_arrays(sd)
    ns = sd.n_spheres
    if name == "mixed5":  # the tall triangle, its upper part: above the ground, behind the dome's reach
        j = [i for i in big if i >= ns][1]
        b = rng.dirichlet([1, 1, 1], 4 * n)
        p = (b @ tri[j - ns])
        p = p[(p[:, 1] > 45) & (p[:, 1] < 100)][:n]
    else:  # nine: the first floor triangle, in the strip between the cluster and the wall at x = 5
        j = [i for i in big if i >= ns][0]
        p = np.stack([rng.uniform(4.75, 4.95, n), np.full(n, 0.05), rng.uniform(-3, 3, n)], axis=1)
    assert len(p) == n
    v = tri[j - ns]
    nrm = np.cross(v[1] - v[0], v[2] - v[0])
    nrm /= np.linalg.norm(nrm)
    side = np.where(rng.random(n) < 0.5, 1.0, -1.0)[:, None] if name == "mixed5" else np.ones((n, 1))
    if name == "nine" and nrm[1] < 0:
        nrm = -nrm
    o = p + side * nrm * 0.25
    return _rays(o, rng.choice([0.0, 0.5, 1.0], n), np.broadcast_to(-side * nrm, (n, 3)) * 1.0, 0.28), j


def cluster_then_outlier_rays(sd, big, rng, n=128):
    """Two waves that meet a peeled hittable in the pre-walk (the floor, straight below) and a nearer cluster sphere in the walk."""
    c, v, r, _, _, _ = pool_arrays(sd)
    small = np.array([i for i in range(sd.n_spheres) if i not in big and r[i] < 1.0])
    k = small[rng.integers(0, len(small), n)]
    time = rng.choice([0.0, 0.5, 1.0], n)
    cen = c[k] + v[k] * time[:, None]
    o = cen + np.stack([rng.uniform(-0.05, 0.05, n), r[k] + 0.3, rng.uniform(-0.05, 0.05, n)], axis=1)
    d = np.stack([rng.uniform(-0.02, 0.02, n), -np.ones(n), rng.uniform(-0.02, 0.02, n)], axis=1)
    return _rays(o, time, d)


def query_rays(oracle, name, t, big, precision, seed=0):
    """-> (rays (n, 8) float64 holding values of the precision, {part: slice}).  The parts beyond ray_mix exist where the scene has
    what they aim at."""
    sd = t.scene_desc()
    rng = np.random.default_rng([seed, sum(map(ord, name)), precision])
    parts = []  # the whole-wave parts first: a wave takes 64 consecutive rays, so each of these fills two waves exactly
    if big:
        parts.append(("cluster_then_outlier", cluster_then_outlier_rays(sd, big, rng)))
    if name in ("mixed5", "nine"):
        parts.append(("only_triangle", only_triangle_rays(name, sd, big, rng)[0]))
    parts.append(("mix", ray_mix(oracle, t, precision, 96, seed=sum(map(ord, name)) + 3)))
    if big:
        a = aimed_rays(sd, big, rng)
        parts.append(("aimed", a))
        parts.append(("tmax", tmax_rays(oracle, sd, big, a, precision)))
    where, at = {}, 0
    for k, p in parts:
        where[k] = slice(at, at + len(p))
        at += len(p)
    return narrow(np.concatenate([p for _, p in parts]), precision), where


def check_designed_parts(name, sd, big, rays, where, idx, oracle, precision):
    """What the designed parts of query_rays() were designed for, asserted on the reference's answers `idx` (mode B, brute force)."""
    if not big:
        assert list(where) == ["mix"]
        return
    ns = sd.n_spheres
    _, t_out, _, _ = brute_force(oracle, _outlier_scene(sd, big), rays, TMIN, precision)
    w = where["cluster_then_outlier"]
    assert w.start % 64 == 0 and w.stop - w.start == 128
    # every lane: an outlier in the pre-walk (ANY may stop there), a nearer cluster sphere in the walk (NEAREST must go on)
    assert np.isfinite(t_out[w]).all() and (idx[w] >= 0).all() and not np.isin(idx[w], big).any()
    if "only_triangle" in where:
        w = where["only_triangle"]
        j = only_triangle_rays(name, sd, big, np.random.default_rng(0))[1]
        assert w.start % 64 == 0 and w.stop - w.start == 128 and j >= ns and j in big
        assert (idx[w] == j).all()
    w = where["aimed"]
    per = (w.stop - w.start) // (2 * len(big))
    a_idx, a_rays = idx[w].reshape(len(big), 2, per), rays[w].reshape(len(big), 2, per, 8)
    hits_some_outlier = np.isfinite(t_out[w]).reshape(len(big), 2, per)
    for k, i in enumerate(big):
        for side in (0, 1):  # from inside the room, from beyond the hittable
            assert hits_some_outlier[k, side].all()
        assert (a_idx[k] == i).any(), (name, i, "never the nearest")
        if kind_of(sd, i) == "m":
            assert set(np.unique(a_rays[k][..., 3])) == {0.0, 0.5, 1.0}
    assert (np.isin(a_idx, big).sum(axis=2) > 0).all()  # both sides of every line find outliers nearest ..
    assert (~np.isin(a_idx, big)).any()  # .. and some rays find the cluster in front of the one they aim at
    inside_wins = sum((a_idx[k, 0] == i).any() for k, i in enumerate(big))
    outside_wins = sum((a_idx[k, 1] == i).any() for k, i in enumerate(big))
    assert inside_wins >= (len(big) + 1) // 2 and outside_wins >= 1, (inside_wins, outside_wins)
    w = where["tmax"]
    tm = rays[w, 7]
    assert np.isfinite(tm).all() and (idx[w] < 0).any() and np.isin(idx[w], big).any()
