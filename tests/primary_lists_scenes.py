"""Scenes of the primary-list tests (tests/test_primary_lists_cpu.py and _gpu.py): frames of 48x27, at most 300
spheres.  Each is a case the beam test (rayz_amd/csrc/primary_lists.hpp: may_hit) can go wrong at; `build(name)` returns the tracer."""
import numpy as np

from rayz_amd import tracer

W, H = 48, 27
K = 32  # primary_lists.hpp: kListK
NO_LIST = 0xFFFFFFFF
# the overflow scene: every pixel of these columns and rows lies behind all 40 spheres of the row along the view axis
OVERFLOW_RECT = (22, 26, 12, 15)  # x0, x1, y0, y1 (exclusive ends)

NAMES = ["defocus_mixed", "pinhole_mixed", "camera_inside_a_sphere", "lens_disc_cuts_a_sphere", "centres_at_3e4", "grazing", "overflow"]


def _tracer(seed, look_from, look_at, defocus_angle=0.0, focus=10.0, vfov=40.0):
    t = tracer.Tracer.init(W, vfov, focus, defocus_angle, look_from, look_at, (0, 1, 0), seed=seed)
    P = t.pool
    rng = np.random.default_rng(seed)
    tex = [P.add_solid_texture(rng.uniform(0.1, 0.9, 3)) for _ in range(4)]
    tex.append(P.add_checker_texture(0.5, tex[0], tex[1]))
    mats = [P.add_diffuse(tex[0], 0), P.add_diffuse(tex[4], 1), P.add_diffuse(tex[2], 2), P.add_metallic(tex[3], 0.0),
            P.add_metallic(tex[1], 0.3), P.add_dielectric(1.5)]
    return t, rng, mats


def _mixed(t, rng, mats, n, centre=(0.0, 0.0, 0.0), spread=8.0, plane=None):
    """n spheres, a third static, a third y-moving, a third generally moving, every fifth with a negative radius; `plane`: the
    static and y-moving ones at that height (plane runs), else at random heights."""
    c0 = np.asarray(centre)
    for k in range(n):
        vel = (0.0, 0.0, 0.0) if k % 3 == 0 else (0.0, float(rng.uniform(0.1, 0.5) * rng.choice([-1, 1])), 0.0) if k % 3 == 1 \
            else tuple(rng.uniform(-0.5, 0.5, 3))
        y = plane if plane is not None and k % 3 != 2 else rng.uniform(-2.0, 3.0)
        c = c0 + (rng.uniform(-spread, spread), y, rng.uniform(-spread, spread))
        r = float(rng.uniform(0.2, 0.5)) * (-1.0 if k % 5 == 4 else 1.0)
        t.pool.add_sphere(tuple(c), r, int(mats[k % len(mats)]), velocity=vel)


def build(name, spp=8, bounces=6):
    if name == "defocus_mixed":  # a lens of radius 0.17 focused at 10
        t, rng, mats = _tracer(101, (0.0, 4.0, 14.0), (0.0, 0.5, 0.0), defocus_angle=2.0)
        t.pool.add_sphere((0.0, -1003.0, 0.0), 1000.0, int(mats[1]))
        _mixed(t, rng, mats, 150, plane=0.4)
    elif name == "pinhole_mixed":
        t, rng, mats = _tracer(102, (3.0, 5.0, 13.0), (0.0, 0.5, 0.0))
        t.pool.add_sphere((0.0, -1003.0, 0.0), 1000.0, int(mats[0]))
        _mixed(t, rng, mats, 150)
    elif name == "camera_inside_a_sphere":  # .. a glass ball of radius 3 about the camera, the pool beyond it
        t, rng, mats = _tracer(103, (0.0, 2.0, 12.0), (0.0, 0.5, 0.0), defocus_angle=1.0)
        t.pool.add_sphere((0.3, 2.2, 11.0), 3.0, int(mats[5]))
        t.pool.add_sphere((0.0, -1003.0, 0.0), 1000.0, int(mats[1]))
        _mixed(t, rng, mats, 90)
    elif name == "lens_disc_cuts_a_sphere":  # the lens (radius 0.26) reaches into a sphere whose surface passes 0.1 from its centre
        t, rng, mats = _tracer(104, (0.0, 2.0, 12.0), (0.0, 0.5, 0.0), defocus_angle=3.0)
        t.pool.add_sphere((0.5, 2.0, 12.0), 0.4, int(mats[3]))
        t.pool.add_sphere((0.0, -1003.0, 0.0), 1000.0, int(mats[1]))
        _mixed(t, rng, mats, 90)
    elif name == "centres_at_3e4":
        far = np.array([3.0e4, 3.0e4, -3.0e4])
        t, rng, mats = _tracer(105, tuple(far + (0.0, 4.0, 14.0)), tuple(far + (0.0, 0.5, 0.0)), defocus_angle=1.0)
        _mixed(t, rng, mats, 150, centre=far, plane=0.4)
    elif name == "grazing":  # 0.3 above the tops of a 10 x 10 field, looking along it
        t, rng, mats = _tracer(106, (0.0, 0.9, 14.0), (0.0, 0.3, 0.0), defocus_angle=0.5)
        t.pool.add_sphere((0.0, -1000.0, 0.0), 1000.0, int(mats[1]))
        for i in range(10):
            for j in range(10):
                vy = 0.0 if (i + j) % 2 else float(rng.uniform(0.1, 0.3))
                t.pool.add_sphere((2.0 * i - 9.0 + rng.uniform(-0.3, 0.3), 0.3, 2.0 * j - 9.0 + rng.uniform(-0.3, 0.3)), 0.3,
                                  int(mats[(i + j) % len(mats)]), velocity=(0.0, vy, 0.0))
    elif name == "overflow":  # 40 glass spheres in a row along the view axis, each 0.08 rad wide: the middle pixels lie behind all of them
        t, rng, mats = _tracer(107, (0.0, 2.0, 14.0), (0.0, 2.0, 0.0))
        t.pool.add_sphere((0.0, -1003.0, 0.0), 1000.0, int(mats[1]))
        for k in range(40):
            dist = 5.0 + 1.5 * k
            t.pool.add_sphere((0.0, 2.0, 14.0 - dist), 0.08 * dist, int(mats[5]))
        _mixed(t, rng, mats, 60)
    elif name == "all_sky":  # the pool lies behind the camera: every list is empty, every path ends in its list phase
        t, rng, mats = _tracer(108, (0.0, 2.0, 14.0), (0.0, 9.0, 30.0))
        _mixed(t, rng, mats, 30)
    else:
        raise KeyError(name)
    t.samples_per_px, t.max_bounces = spp, bounces
    t.set_gpu(render_seed=int(rng.integers(0, 2 ** 62)))
    p = t.params()
    assert (p.width, p.height) == (W, H), (p.width, p.height)
    return t


def camera_row(c):
    """The camera as tests/primary_lists_mirror.cpp reads it."""
    return np.array(list(c.look_from) + list(c.px_du) + list(c.px_dv) + list(c.px_origin) + list(c.defocus_u) + list(c.defocus_v) + [float(c.defocus)])
