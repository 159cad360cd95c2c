"""Plane runs of the flat list's scan on the device.

1. The run form itself: RAYZ_KAT_SCAN_DISCS classes 2 / 3 run ScanGroup<float, 3 / 4>::discs with K2 put in the basis as
   scan_plane_class does.  Held bit for bit to the CPU mirror (tests/plane_filter_mirror.cpp `discs`, from the padded r²
   the library returns), and to the f64 discriminant of mode A: no false negative on plane blocks, config-3 segments and
   the adversarial / 3e4-shifted sphere records.
2. Run layouts that randomBouncing never makes (its grid is ONE run per class, at first = 0): several runs per class, more
   qualifying heights than runs, runs ending off whole group pairs, runs in one class only, classes of runs only or of
   loose spheres only, ±0 and negative heights, heights at 3e4, f64 heights that are one f32 height, more candidates in a
   run than a lane parks, duplicate spheres inside a run.  Each scene first asserts, through the mirror's `layout`, that it
   forms exactly the runs it was built for; then the flat list (forced: AUTO picks the BVH for these pools) is held to
   oracle mode B bit for bit, segments included, and to the device's BVH frame, in f32 and f64."""
import numpy as np
import pytest

import kat_records as K
from helpers import assert_images_equal
from rayz_amd import capi, tracer
from test_kat_cpu import _bad_scan_records
from test_plane_runs import _config3_segments, _run, _spheres, _write, mirror, mirror_discs  # noqa: F401  (mirror: a fixture)

pytestmark = pytest.mark.gpu

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR, BVH = capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH
SCAN = capi.KAT_SCAN_DISCS


def bits32(x):
    return int(np.float32(x).view(np.uint32))


# ---- 1. the run form ---------------------------------------------------------------------------------------------------
def _same_bits(a, b):
    return np.asarray(a, dtype=np.float32).view(np.uint32) == np.asarray(b, dtype=np.float32).view(np.uint32)


def _check_plane_form(gpu, oracle, mirror, tmp_path, rec, prec, what, band=None):
    """Device vs mirror (bit for bit), vs the library's r² rule, vs mode B's leaf form, vs mode A (no false negative)."""
    rec = rec.copy()
    rec[:, 32] = 1.0  # want_r2: the padded r² the library used comes back in out[8..11]
    got = gpu.kat(SCAN, rec, prec)
    assert np.array_equal(got[:, 8:12], K.scan_pad_r2(rec, prec)), what
    r = rec.copy()
    r[:, 28:32] = got[:, 8:12]
    m = mirror_discs(mirror, tmp_path, r, prec)
    same = _same_bits(got[:, :4], m[:, :4])
    assert same.all(), (what, prec, int((~same).any(1).sum()), np.flatnonzero(~same.all(1))[:5].tolist())
    assert not (m[:, 4:] >= 0).any(), what  # a pad slot (r² = -inf) at any place of the block never passes
    b = oracle.kat_b(SCAN, rec, prec)
    assert np.array_equal(got[:, 4:], b[:, 4:]), what  # the leaf form and r² are mode B's
    a = oracle.kat_a(SCAN, rec)[:, :4]
    hit = a >= 0
    assert hit.any() and (got[:, :4][hit] >= 0).all(), (what, prec, int((got[:, :4][hit] < 0).sum()))
    if band:
        assert band[0] < (got[:, :4] >= 0).mean() < band[1], what
    return got


@pytest.mark.parametrize("prec", [F32, F64])
def test_device_plane_form_on_plane_blocks(gpu, oracle, mirror, tmp_path, prec):
    rec = K.random_plane_blocks(np.random.default_rng(8), 200_000)
    got = _check_plane_form(gpu, oracle, mirror, tmp_path, rec, prec, "plane blocks", band=(0.1, 0.6))
    assert np.isfinite(got[:, :8]).all()
    # the run form and the loose form filter alike but round differently: they must not be one code path
    loose = rec.copy()
    loose[:, 27] -= 2
    assert not np.array_equal(gpu.kat(SCAN, loose, prec)[:, :4], got[:, :4])


def _run_blocks(sph, rays, f64_rays):
    """KAT records of config 3's two plane runs (cy = 0.2, static and y-moving) against its segments: per ray and class,
    the 8 run members nearest to the ray's line at the ray's time, as two blocks of 4."""
    static = (sph[:, 3:6] == 0).all(1) & (np.float32(sph[:, 1]) == np.float32(0.2))
    movy = (sph[:, 3] == 0) & (sph[:, 5] == 0) & (sph[:, 4] != 0) & (np.float32(sph[:, 1]) == np.float32(0.2))
    out = []
    for cls, sel in ((2.0, static), (3.0, movy)):
        idx = np.flatnonzero(sel)
        for lo in range(0, len(rays), 2000):
            ry = rays[lo:lo + 2000]
            c = sph[idx, None, 0:3] + sph[idx, None, 3:6] * ry[None, :, 6:7]  # (members, rays, 3)
            oc = c - ry[None, :, 0:3]
            d = K.unit(ry[:, 3:6])[None]
            dist = np.linalg.norm(oc - (oc * d).sum(2, keepdims=True) * d, axis=2) - sph[idx, None, 6]
            near = idx[np.argsort(dist, axis=0)[:8]].T  # (rays, 8)
            for half in (near[:, :4], near[:, 4:]):
                rec = K.blank(len(ry))
                s = sph[half]  # (rays, 4, 7)
                rec[:, 0:4], rec[:, 4:8], rec[:, 8:12], rec[:, 12:16], rec[:, 16:20] = s[..., 0], s[..., 1], s[..., 2], s[..., 6], s[..., 4]
                rec[:, 20:23], rec[:, 23:26], rec[:, 26], rec[:, 27] = ry[:, 0:3], ry[:, 3:6], ry[:, 6], cls
                out.append(rec)
    rec = np.concatenate(out)
    if not f64_rays:
        rec[:, 20:27] = K.f32r(rec[:, 20:27])
    return rec


@pytest.mark.parametrize("prec", [F32, F64])
def test_device_plane_form_on_config3_segments(gpu, oracle, mirror, tmp_path, prec):
    sph, rays, _ = _config3_segments(np.random.default_rng(5), n_primary=2000, n_bounce=6000)
    rec = _run_blocks(sph, rays, prec == F64)
    got = _check_plane_form(gpu, oracle, mirror, tmp_path, rec, prec, "config-3 segments")
    assert (oracle.kat_a(SCAN, rec)[:, :4] >= 0).sum() > 3000 and (got[:, :4] >= 0).mean() < 0.6


@pytest.mark.parametrize("prec", [F32, F64])
def test_device_plane_form_on_grazing_rays_and_big_coordinates(gpu, oracle, mirror, tmp_path, prec):
    """test_plane_runs.py's adversarial (ray, sphere) records, each sphere its own run (all four slots of the block)."""
    rng = np.random.default_rng(9)
    for shift in (0.0, 3.0e4):
        h = K.random_sphere_hits(rng, 40_000, big=True)
        h[:, 0:3] = K.f32r(h[:, 0:3] + shift)
        h[:, 7:10] = K.f32r(h[:, 7:10] + shift)
        h = h[(h[:, 3] == 0) & (h[:, 5] == 0)]
        rec = K.blank(len(h))
        for k in range(4):
            rec[:, k], rec[:, 4 + k], rec[:, 8 + k], rec[:, 12 + k], rec[:, 16 + k] = h[:, 0], h[:, 1], h[:, 2], h[:, 6], h[:, 4]
        rec[:, 20:23], rec[:, 23:26], rec[:, 26] = h[:, 7:10], h[:, 10:13], h[:, 13]
        rec[:, 27] = np.where(h[:, 4] == 0, 2.0, 3.0)
        _check_plane_form(gpu, oracle, mirror, tmp_path, rec, prec, f"sphere hits shifted {shift}")


def test_kat_refuses_bad_scan_records(gpu):
    """The library refuses what the oracle refuses (test_kat_cpu.py: test_scan_discs_argument_checks_on_the_oracle)."""
    for why, rec in _bad_scan_records():
        with pytest.raises(capi.RayzHipError, match="class|cy|want_r2"):
            gpu.kat(SCAN, rec)
    rec = K.random_plane_blocks(np.random.default_rng(4), 8)
    rec[:, 4:8] = 0.7 + np.array([0.0, 1e-12, -1e-12, 3e-9])  # one f32 height, four f64 ones
    for cls in (0.0, 1.0, 2.0, 3.0):
        rec[:, 27] = cls
        gpu.kat(SCAN, rec, F64)


# ---- 2. run layouts rendered ---------------------------------------------------------------------------------------------
GROUND_TOP = -4.0  # below every height the layouts use, so that negative heights are in view


class Scene:
    """A pool built sphere by sphere: `group` adds N spheres of one class at one height (a run if N >= 64 and among its class's
    four largest), `loose` spheres at random heights, mov-G spheres, a ground sphere; mixed materials.  The pool order is
    shuffled at build() (duplicates added after it keep their place at the end)."""

    def __init__(self, seed, look_from=(0.0, 7.0, 15.0), look_at=(0.0, 1.0, 0.0), width=48, y0=0.0, ground_vy=0.0):
        self.rng = np.random.default_rng(seed)
        self.t = tracer.Tracer.init(width, 40.0, 10.0, 0.0, look_from, look_at, (0, 1, 0), seed=seed)
        P = self.t.pool
        rng = self.rng
        tex = [P.add_solid_texture(rng.uniform(0.1, 0.9, 3)) for _ in range(4)]
        tex.append(P.add_checker_texture(0.5, tex[0], tex[1]))
        self.mats = [P.add_diffuse(tex[0], 0), P.add_diffuse(tex[4], 1), P.add_diffuse(tex[2], 2), P.add_metallic(tex[3], 0.0),
                     P.add_metallic(tex[1], 0.3), P.add_dielectric(1.5)]
        self.y0 = y0
        self.rows = [((0.0, y0 + GROUND_TOP - 1000.0, 0.0), 1000.0, self.mats[1], (0.0, ground_vy, 0.0))]
        self.tail = []

    def sphere(self, c, r, vel=(0.0, 0.0, 0.0), mat=None):
        self.rows.append((tuple(c), float(r), int(self.rng.choice(self.mats)) if mat is None else mat, tuple(vel)))

    def group(self, cls, cy, n, spread=8.0, r=(0.2, 0.45)):
        for _ in range(n):
            vy = float(self.rng.uniform(0.1, 0.6) * self.rng.choice([-1, 1])) if cls else 0.0
            y = cy() if callable(cy) else cy if self.y0 == 0 else self.y0 + cy  # (0.0 + -0.0 would be +0.0)
            c = (self.rng.uniform(-spread, spread), y, self.rng.uniform(-spread, spread))
            self.sphere(c, self.rng.uniform(*r), (0.0, vy, 0.0))
        return self

    def loose(self, n_static=8, n_movy=8, n_movg=6):
        rng = self.rng
        for k in range(n_static + n_movy + n_movg):
            vel = ((0.0, 0.0, 0.0) if k < n_static else (0.0, float(rng.uniform(-0.5, 0.5)) or 0.1, 0.0) if k < n_static + n_movy
                   else tuple(rng.uniform(-0.5, 0.5, 3)))
            self.sphere((rng.uniform(-8, 8), self.y0 + rng.uniform(-3.0, 3.5), rng.uniform(-8, 8)), rng.uniform(0.2, 0.8), vel)
        return self

    def build(self, spp=8, bounces=6):
        P = self.t.pool
        order = self.rng.permutation(len(self.rows))
        for i in order:
            c, r, m, v = self.rows[i]
            P.add_sphere(c, r, m, velocity=v)
        for c, r, m, v in self.tail:
            P.add_sphere(c, r, m, velocity=v)
        self.t.samples_per_px, self.t.max_bounces = spp, bounces
        self.t.set_gpu(render_seed=int(self.rng.integers(0, 2 ** 62)))
        return self.t


def assert_layout(mirror, tmp_path, t, want):
    """The scene forms exactly the runs it was built for: want = {class: [(cy, members), ...] in layout order}; a class not
    named has no run.  Checks the slots too: runs back to back from 0, each padded to whole group pairs."""
    sph = _spheres(t)
    lay = _run(mirror, tmp_path, "layout", _write(tmp_path, "s.bin", sph))
    for c in (0, 1):
        cl = lay["classes"][c]
        got = [(bits32(sph[r["members"][0], 1]), len(r["members"])) for r in cl["runs"]]
        assert got == [(bits32(cy), n) for cy, n in want.get(c, [])], (c, got, want.get(c))
        at = 0
        for r in cl["runs"]:
            assert r["first"] == at and r["end"] - r["first"] == -(-len(r["members"]) // 8) * 8
            at = r["end"]
        assert cl["plane_slots"] == at
    return lay


def check_frames(gpu, oracle, t, what):
    """Flat list (forced) == oracle mode B bit for bit, segments equal; the BVH frame == the flat list's; both precisions."""
    for prec in (F32, F64):
        t.set_gpu(traversal=LINEAR, precision=prec)
        scene, cam, p = t.scene_desc(), t.camera_desc(), t.params()
        got, gst = gpu.render_host(scene, cam, p)
        want, ost = oracle.render_b(scene, cam, p)
        assert_images_equal(got, want, f"{what}: flat list, precision {prec}")
        assert gst.segments == ost.segments, (what, prec)
        t.set_gpu(traversal=BVH)
        got_b, bst = gpu.render_host(t.scene_desc(), t.camera_desc(), t.params())
        assert_images_equal(got_b, got, f"{what}: BVH vs flat list, precision {prec}")
        assert bst.segments == gst.segments, (what, prec)


def _layout(name):
    """(scene, the runs it must form) for each named layout."""
    if name.startswith("static_runs_"):
        k = int(name[-1])
        hs = [0.4, 1.3, 2.2, 3.1][:k]
        s = Scene(10 + k)
        for j, h in enumerate(hs):
            s.group(0, h, 64 + 5 * j)
        return s.loose(), {0: [(h, 64 + 5 * j) for j, h in enumerate(hs)]}
    if name == "five_heights":  # the 64s tie: 1.5 (0x3fc00000) beats -0.5 (0xbf000000), which stays loose
        s = Scene(20)
        for h, n in [(1.5, 64), (-0.5, 64), (2.5, 90), (0.5, 80), (3.5, 70)]:
            s.group(0, h, n)
        return s.loose(), {0: [(0.5, 80), (1.5, 64), (2.5, 90), (3.5, 70)]}
    if name == "six_heights":  # in mov-Y; -0.0 beats -2.0 at 65 by bits, but both outsize the 64s
        s = Scene(21)
        for h, n in [(0.25, 100), (-2.0, 65), (0.75, 64), (1.25, 72), (3.0, 64), (-0.0, 65)]:
            s.group(1, h, n)
        s.group(0, 2.0, 64)
        return s.loose(), {0: [(2.0, 64)], 1: [(-2.0, 65), (-0.0, 65), (0.25, 100), (1.25, 72)]}
    if name == "member_counts":  # runs ending on and off whole group pairs, pad slots between runs, 63 stays loose
        s = Scene(22)
        for h, n in [(0.3, 63), (0.9, 64), (1.5, 65), (2.1, 71), (2.7, 72)]:
            s.group(0, h, n)
        for h, n in [(0.6, 73), (1.8, 64), (2.4, 63)]:
            s.group(1, h, n)
        return s.loose(), {0: [(0.9, 64), (1.5, 65), (2.1, 71), (2.7, 72)], 1: [(0.6, 73), (1.8, 64)]}
    if name == "static_only":
        return Scene(23).group(0, 0.5, 70).group(0, 1.5, 66).loose(), {0: [(0.5, 70), (1.5, 66)]}
    if name == "movy_only":
        return Scene(24).group(1, 0.5, 70).group(1, 1.5, 66).loose(), {1: [(0.5, 70), (1.5, 66)]}
    if name == "both_classes":
        return Scene(25).group(0, 0.5, 70).group(1, 0.5, 66).group(1, 1.7, 65).loose(), {0: [(0.5, 70)], 1: [(0.5, 66), (1.7, 65)]}
    if name == "runs_only_and_loose_only":  # static: runs and nothing else (the ground moves in y); mov-Y: loose only
        s = Scene(26, ground_vy=1e-3).group(0, 0.5, 64).group(0, 1.4, 72)
        return s.loose(n_static=0), {0: [(0.5, 64), (1.4, 72)]}
    if name == "loose_only_and_runs_only":  # the other way round
        s = Scene(27).group(1, 0.5, 64).group(1, 1.4, 72)
        return s.loose(n_movy=0), {1: [(0.5, 64), (1.4, 72)]}
    if name == "signed_zeros_and_negatives":  # +0 and -0: two runs, +0 first; negative heights; the camera low and near
        s = Scene(28, look_from=(0.0, 2.0, 11.0), look_at=(0.0, -0.5, 0.0))
        s.group(0, 0.0, 64).group(0, -0.0, 65).group(0, -1.5, 66).group(1, -0.7, 64).group(1, -0.0, 64)
        return s.loose(), {0: [(-1.5, 66), (0.0, 64), (-0.0, 65)], 1: [(-0.7, 64), (-0.0, 64)]}
    if name == "far_3e4":  # everything 3e4 up (f32 spacing there: 2^-9), the camera near it
        y0 = 3.0e4
        s = Scene(29, look_from=(0.0, y0 + 6.0, 14.0), look_at=(0.0, y0 + 1.0, 0.0), y0=y0)
        s.group(0, 0.5, 64).group(0, 1.5, 70).group(1, 1.0, 66)
        return s.loose(), {0: [(y0 + 0.5, 64), (y0 + 1.5, 70)], 1: [(y0 + 1.0, 66)]}
    if name == "f64_heights_one_f32":  # f64 heights that differ, one f32 height: one run; the narrow phase sees the f64 ones
        s = Scene(30)
        h32 = float(np.float32(0.7))
        s.group(0, lambda: h32 + s.rng.uniform(-1e-8, 1e-8), 80).group(1, lambda: h32 + s.rng.uniform(-1e-8, 1e-8), 70)
        assert len({r[0][1] for r in s.rows[1:]}) > 100
        return s.loose(), {0: [(h32, 80)], 1: [(h32, 70)]}
    if name == "row_view":  # along a row of overlapping spheres at one height: more than 4 candidates per lane in the run
        s = Scene(31, look_from=(-12.0, 1.0, 0.0), look_at=(10.0, 1.0, 0.0), width=32)
        for k in range(96):
            s.sphere((-4.0 + 0.12 * k, 1.0, 0.15 * np.sin(k)), 0.45)
        s.group(0, 0.2, 66)
        return s.loose(), {0: [(0.2, 66), (1.0, 96)]}
    if name == "duplicates":  # identical spheres in one run far apart in pool order: the larger pool index wins the tie
        s = Scene(32)
        s.group(0, 0.8, 80, spread=3.0, r=(0.5, 0.8))
        for c, r, m, v in s.rows[1:21]:  # copies with another material, after the whole shuffled pool
            s.tail.append((c, r, s.mats[3] if m != s.mats[3] else s.mats[0], v))
        return s.loose(n_static=2), {0: [(0.8, 100)]}
    raise KeyError(name)


LAYOUTS = ["static_runs_2", "static_runs_3", "static_runs_4", "five_heights", "six_heights", "member_counts", "static_only",
           "movy_only", "both_classes", "runs_only_and_loose_only", "loose_only_and_runs_only", "signed_zeros_and_negatives",
           "far_3e4", "f64_heights_one_f32", "row_view", "duplicates"]


@pytest.mark.parametrize("name", LAYOUTS)
def test_run_layout_renders_like_the_oracle(gpu, oracle, mirror, tmp_path, name):
    s, want = _layout(name)
    t = s.build()
    assert_layout(mirror, tmp_path, t, want)
    check_frames(gpu, oracle, t, name)


def test_duplicates_in_a_run_hit_the_later_copy(gpu, oracle):
    """The duplicate layout's ties are real and go to the copy: giving the originals the copies' materials changes nothing
    (the device's flat-list frame == mode B's frame of that pool), removing the copies changes the frame."""
    t = _layout("duplicates")[0].build()
    t.set_gpu(traversal=LINEAR, precision=F32)
    got, _ = gpu.render_host(t.scene_desc(), t.camera_desc(), t.params())
    s2 = _layout("duplicates")[0]
    for k, (c, r, m, v) in enumerate(s2.tail):
        s2.rows[1 + k] = (c, r, m, v)  # the originals in the copies' materials: whichever wins, the same frame
    t2 = s2.build()
    t2.set_gpu(traversal=LINEAR, precision=F32)
    assert_images_equal(got, oracle.render_b(t2.scene_desc(), t2.camera_desc(), t2.params())[0], "originals in the copies' materials")
    s3 = _layout("duplicates")[0]
    s3.tail = []
    t3 = s3.build()
    t3.set_gpu(traversal=LINEAR, precision=F32)
    assert not np.array_equal(got, oracle.render_b(t3.scene_desc(), t3.camera_desc(), t3.params())[0])


def test_device_scene_with_runs_through_near_far_near(gpu, oracle, mirror, tmp_path):
    """One DeviceScene with runs in both classes: near camera, a camera 20,000 units out (the larger origin bound re-pads the
    plane streams), near again; f32 and f64; every step held to the oracle (tests/test_reuse_gpu.py's pattern)."""
    from test_reuse_gpu import FAR, Want, camera, params, render_checked

    s, want = _layout("member_counts")
    t = s.build()
    assert_layout(mirror, tmp_path, t, want)
    scene = t.scene_desc()
    w = Want(oracle, scene)
    near = camera(oracle, ((0.0, 7.0, 15.0), 40.0, 10.0), 48, 27)
    far = camera(oracle, FAR, 64, 36)
    ds = gpu.DeviceScene(scene)
    try:
        for prec in (F32, F64):
            for cam, wh, tag in ((near, (48, 27), "near"), (far, (64, 36), "far"), (near, (48, 27), "near again")):
                p = params(t.params(), width=wh[0], height=wh[1], traversal=LINEAR, precision=prec)
                render_checked(ds, w, cam, p, f"{tag}, precision {prec}")
    finally:
        ds.close()
