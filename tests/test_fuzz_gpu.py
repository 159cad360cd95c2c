"""Randomised scenes: every hittable class (static / y-moving / generally moving spheres, triangles), every
material and texture kind, random cameras (with and without defocus) — GPU vs oracle mode B, bit for bit, in both
precisions and both traversals."""
import numpy as np
import pytest

from helpers import assert_images_equal
from rayz_amd import capi, tracer

pytestmark = pytest.mark.gpu


def random_scene(seed):
    rng = np.random.default_rng(seed)
    look_from = rng.uniform(-6, 6, 3) + np.array([0, 3.0, 0])
    t = tracer.Tracer.init(int(rng.integers(24, 72)), float(rng.uniform(20, 70)), float(rng.uniform(2, 10)),
                           float(rng.choice([0.0, 0.0, 1.0, 3.0])), look_from, rng.uniform(-1, 1, 3), (0, 1, 0), seed=seed)
    P = t.pool
    tex = [P.add_solid_texture(rng.uniform(0.05, 0.95, 3)) for _ in range(4)]
    tex.append(P.add_checker_texture(float(rng.uniform(0.1, 1.0)), tex[0], tex[1]))
    tex.append(P.add_checker_texture(float(rng.uniform(0.3, 2.0)), tex[4], tex[2]))
    mats = []
    for k in range(10):
        kind = rng.integers(0, 3)
        if kind == 0:
            mats.append(P.add_diffuse(int(rng.choice(tex)), int(rng.integers(0, 3))))
        elif kind == 1:
            mats.append(P.add_metallic(int(rng.choice(tex)), float(rng.choice([0.0, rng.uniform(0, 1.5)]))))
        else:
            mats.append(P.add_dielectric(float(rng.choice([1.5, 1.33, 1 / 1.5, 2.4]))))
    P.add_sphere((0, -500, 0), 500.0, mats[0])
    for _ in range(int(rng.integers(0, 40))):
        cls = rng.integers(0, 3)
        v = (0, 0, 0) if cls == 0 else ((0, float(rng.uniform(-1, 1)), 0) if cls == 1 else tuple(rng.uniform(-1, 1, 3)))
        c = rng.uniform(-4, 4, 3)
        c[1] = abs(c[1]) * 0.5 + 0.2
        P.add_sphere(c, float(rng.uniform(0.1, 0.9)), int(rng.choice(mats)), velocity=v)
    for _ in range(int(rng.integers(0, 30))):
        base = rng.uniform(-4, 4, 3)
        base[1] = abs(base[1]) * 0.5
        P.add_triangle(base, base + rng.uniform(-1.5, 1.5, 3), base + rng.uniform(-1.5, 1.5, 3), int(rng.choice(mats)))
    t.samples_per_px = int(rng.integers(1, 20))
    t.max_bounces = int(rng.integers(1, 30))
    t.set_gpu(render_seed=int(rng.integers(0, 2 ** 62)), chunk_spp=int(rng.choice([0, 1, 3, 16])))
    return t


def axis_scene(seed):
    """Second generator: the geometry that makes exact zeros and ties — axis-aligned quads and boxes on integer
    coordinates, spheres centred on lattice points (some far from the origin, where a small scatter offset is absorbed
    by rounding), mirrors and glass, a camera that may look straight down an axis."""
    rng = np.random.default_rng(seed)
    far = float(rng.choice([0.0, 0.0, 100.0, 3000.0]))  # offset of the whole scene along x
    axis_cam = rng.random() < 0.5
    look_from = np.array([far, 2.0, 8.0]) if axis_cam else rng.uniform(-6, 6, 3) + np.array([far, 3.0, 0])
    look_at = np.array([far, 2.0, 0.0]) if axis_cam else np.array([far, 1.0, 0.0]) + rng.uniform(-1, 1, 3)
    t = tracer.Tracer.init(int(rng.integers(24, 64)), float(rng.uniform(20, 70)), float(rng.uniform(2, 10)),
                           float(rng.choice([0.0, 0.0, 1.0])), look_from, look_at, (0, 1, 0), seed=seed)
    P = t.pool
    tex = [P.add_solid_texture(rng.uniform(0.05, 0.95, 3)) for _ in range(3)]
    tex.append(P.add_checker_texture(1.0, tex[0], tex[1]))
    mats = [P.add_diffuse(int(rng.choice(tex)), 2), P.add_diffuse(int(rng.choice(tex)), int(rng.integers(0, 3))),
            P.add_metallic(tex[0], 0.0), P.add_metallic(tex[1], 0.3), P.add_dielectric(1.5), P.add_dielectric(1 / 1.5)]
    P.add_sphere((far, -500, 0), 500.0, int(rng.choice(mats)))  # the ground: sometimes glass or a mirror
    for _ in range(int(rng.integers(0, 20))):
        c = np.round(rng.uniform(-4, 4, 3))
        c[1] = abs(c[1]) + 1.0
        c[0] += far
        v = (0, 0, 0) if rng.random() < 0.6 else (0, float(rng.choice([0.5, -0.25, 1.0])), 0)
        P.add_sphere(c, float(rng.choice([0.5, 1.0, 0.25])), int(rng.choice(mats)), velocity=v)

    def quad(a, e1, e2, m):
        P.add_triangle(a, a + e1, a + e1 + e2, m)
        P.add_triangle(a, a + e1 + e2, a + e2, m)

    for _ in range(int(rng.integers(0, 6))):  # axis-aligned boxes and single quads
        lo = np.round(rng.uniform(-4, 3, 3))
        lo[1] = abs(lo[1])
        lo[0] += far
        sz = rng.choice([1.0, 2.0, 0.5], 3)
        m = int(rng.choice(mats))
        ex, ey, ez = np.array([sz[0], 0, 0]), np.array([0, sz[1], 0]), np.array([0, 0, sz[2]])
        if rng.random() < 0.5:
            quad(lo, ex, ey, m), quad(lo + ez, ex, ey, m), quad(lo, ex, ez, m), quad(lo + ey, ex, ez, m)
            quad(lo, ey, ez, m), quad(lo + ex, ey, ez, m)
        else:
            quad(lo, *[(ex, ey), (ex, ez), (ey, ez)][int(rng.integers(0, 3))], m)
    t.samples_per_px = int(rng.integers(1, 16))
    t.max_bounces = int(rng.integers(2, 40))
    t.set_gpu(render_seed=int(rng.integers(0, 2 ** 62)), chunk_spp=int(rng.choice([0, 1, 16])))
    return t


def plane_scene(seed):
    """Third generator: plane runs, which the two above never form (at most 40 spheres, random heights).  1 to 6
    heights (+0, -0, negative or positive), 40 / 63 / 64 / 65 / 100 / 257 spheres each, static or y-moving per height,
    among loose, generally moving spheres and a ground sphere; random materials; a camera that may sit at a run's height
    and look horizontally along it."""
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


@pytest.mark.parametrize("seed", range(300, 308))
def test_plane_scene_parity(gpu, oracle, seed):
    """Flat list == oracle mode B and == the BVH frame, bit for bit, segments equal, in both precisions."""
    t = plane_scene(seed)
    for prec in (capi.PRECISION_F32, capi.PRECISION_F64):
        t.set_gpu(traversal=capi.TRAVERSAL_LINEAR, precision=prec)
        scene, cam, p = t.scene_desc(), t.camera_desc(), t.params()
        got, gst = gpu.render_host(scene, cam, p)
        want, ost = oracle.render_b(scene, cam, p)
        assert_images_equal(got, want, f"plane scene {seed} precision {prec}")
        assert gst.segments == ost.segments
        t.set_gpu(traversal=capi.TRAVERSAL_BVH)
        got_b, bst = gpu.render_host(t.scene_desc(), t.camera_desc(), t.params())
        assert_images_equal(got_b, got, f"plane scene {seed} precision {prec}: BVH vs flat list")
        assert bst.segments == gst.segments


@pytest.mark.parametrize("seed", range(200, 208))
def test_axis_scene_parity(gpu, oracle, seed):
    t = axis_scene(seed)
    for trav in (capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH):
        for prec in (capi.PRECISION_F32, capi.PRECISION_F64):
            t.set_gpu(traversal=trav, precision=prec)
            scene, cam, p = t.scene_desc(), t.camera_desc(), t.params()
            got, gst = gpu.render_host(scene, cam, p)
            want, ost = oracle.render_b(scene, cam, p)
            assert_images_equal(got, want, f"axis scene {seed} traversal {trav} precision {prec}")
            assert gst.segments == ost.segments


@pytest.mark.parametrize("seed", range(6))
def test_big_scene_flat_list_equals_bvh(gpu, oracle, seed):
    """tools/fuzz_big.py's generator (200-3,000 spheres, triangles, an oversized ground or not: trees deeper than the
    LDS copy of their top): flat list == BVH exactly on the device in both precisions; one scene against the oracle."""
    import importlib.util
    import os

    spec = importlib.util.spec_from_file_location("fuzz_big_gen", os.path.join(os.path.dirname(__file__), "..", "tools", "fuzz_big.py"))
    src = open(spec.origin).read().split("first, count = int(sys.argv[1])")[0]  # the generator, not the campaign loop
    ns = {"__file__": spec.origin}
    exec(compile(src, spec.origin, "exec"), ns)
    t = ns["big_scene"](seed)
    for prec in (capi.PRECISION_F32, capi.PRECISION_F64):
        got = {}
        for trav in (capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH):
            t.set_gpu(traversal=trav, precision=prec)
            got[trav] = gpu.render_host(t.scene_desc(), t.camera_desc(), t.params())
        a, b = got[capi.TRAVERSAL_LINEAR], got[capi.TRAVERSAL_BVH]
        assert np.array_equal(a[0], b[0], equal_nan=True) and a[1].segments == b[1].segments, (seed, prec)
        if seed == 0:
            want, ost = oracle.render_b(t.scene_desc(), t.camera_desc(), t.params())
            assert_images_equal(b[0], want, f"big scene {seed} precision {prec}")
            assert b[1].segments == ost.segments


# 1000..1011, and three scenes on which the BVH walk once lost hits to a zero direction component (tests/test_kat_cpu.py)
@pytest.mark.parametrize("seed", list(range(1000, 1012)) + [5003, 5008, 5010])
def test_random_scene_parity(gpu, oracle, seed):
    t = random_scene(seed)
    for trav in (capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH):
        for prec in (capi.PRECISION_F32, capi.PRECISION_F64):
            t.set_gpu(traversal=trav, precision=prec)
            scene, cam, p = t.scene_desc(), t.camera_desc(), t.params()
            got, gst = gpu.render_host(scene, cam, p)
            want, ost = oracle.render_b(scene, cam, p)
            assert_images_equal(got, want, f"seed {seed} traversal {trav} precision {prec}")
            assert gst.segments == ost.segments
