"""The flat list's XY-basis kernel (flat_xy_kernel: 5 packed FMAs per sphere pair in plane runs and speed buckets; DESIGN.md §4.3,
§6) on the device.

1. The device's XY forms, RAYZ_KAT_SCAN_DISCS_XY / RAYZ_KAT_BUCKET_DISCS_XY (make_basis<float, kBasisXY>, the run's and bucket's
   K1 / K2, the 5 / 7 / 9-FMA discs), bit for bit against the CPU mirror (tests/flat_xy_mirror.cpp `discs`): the discs, the two
   constants and e1, on loose, run and bucket blocks and on the directions that reach the basis's corners (along ±z exactly, h²
   below and just above 1e-30, along y, along x, level with the run); f32 and f64.
2. Renders at the smallest scenes the loops can go wrong at, 32x18 at 4 spp: the form AUTO chose is asserted (against the mirror's
   `form` of the same pool), then the scene is rendered with AUTO, XZ and XY, each frame held bit for bit to oracle mode B (segments
   too) and the BVH frame to them; f32 and f64."""
import subprocess

import numpy as np
import pytest

import kat_records as K
from helpers import assert_images_equal
from rayz_amd import capi, tracer
from test_flat_xy import xmirror  # noqa: F401  (a fixture)
from test_plane_runs import _run, _spheres, _write
from test_plane_runs_gpu import Scene, _layout
from test_reuse_gpu import FAR, Want, camera, out_tensor, params, render_checked
from test_speed_buckets_gpu import _bucket_layout, bucket_blocks, bucket_group, bucket_pad_r2, f64_disc

pytestmark = pytest.mark.gpu

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR, BVH = capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH
AUTO, XZ, XY = capi.SCAN_FORM_AUTO, capi.SCAN_FORM_XZ, capi.SCAN_FORM_XY
f32 = np.float32


def bits(x):
    return np.asarray(x, dtype=f32).view(np.uint32)


# ---- 1. the XY forms ---------------------------------------------------------------------------------------------------------
def corner_directions(rec, rng):
    """The records' rays turned to the XY basis's corners, in six equal parts: along ±z exactly; |d.x|, |d.y| about 1e-16 beside
    d.z = ±1 (h² about 1e-32: the fallback e1 = (1, 0, 0)); h² just above 1e-30; along ±y; along ±x; level with the block's first
    sphere (o.y = cy, d.y = 0).  The origin is put on the line through a point near sphere 0's rim."""
    rec = rec.copy()
    n = len(rec)
    kind = np.arange(n) * 6 // n
    sgn = rng.choice([-1.0, 1.0], n)
    d = np.zeros((n, 3))
    z = kind <= 2
    d[z, 2] = sgn[z]
    d[kind == 1, 0] = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.5e-16, 2e-16, n))[kind == 1]
    d[kind == 1, 1] = (rng.choice([-1.0, 1.0], n) * rng.uniform(0.5e-16, 2e-16, n))[kind == 1]
    d[kind == 2, 0] = (rng.choice([-1.0, 1.0], n) * 1e-15 * rng.uniform(1.0000001, 1.1, n))[kind == 2]
    d[kind == 3, 1] = sgn[kind == 3]
    d[kind == 4, 0] = sgn[kind == 4]
    a = rng.uniform(0, 2 * np.pi, n)
    d[kind == 5, 0], d[kind == 5, 2] = np.cos(a)[kind == 5], np.sin(a)[kind == 5]
    dn = K.unit(d)
    off = rng.normal(size=(n, 3))
    off -= (off * dn).sum(1, keepdims=True) * dn
    off = K.unit(off) * (rec[:, 12] * rng.uniform(0.9, 1.1, n))[:, None]
    off[kind == 5, 1] = 0.0
    c0 = np.stack([rec[:, 0], rec[:, 4], rec[:, 8]], 1)
    rec[:, 20:23] = K.f32r(c0 + off - dn * rng.uniform(1, 40, (n, 1)))
    rec[kind == 5, 21] = rec[kind == 5, 4]
    rec[:, 23:26] = d * rng.choice([0.5, 1.0, 2.0], (n, 1))
    return rec


def mirror_xy(xmirror, tmp_path, rec, prec, op):
    p = _write(tmp_path, "rec.bin", rec)
    r = subprocess.run([xmirror, "discs", str(p), str(int(prec == F64)), str(op)], capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return np.frombuffer(r.stdout, dtype=f32).reshape(-1, 8)


@pytest.mark.parametrize("prec", [F32, F64])
def test_device_xy_forms_equal_the_mirror(gpu, xmirror, tmp_path, prec):
    rng = np.random.default_rng(31)
    loose, plane = K.random_scan_blocks(rng, 120), K.random_plane_blocks(rng, 120)
    rec = np.concatenate([loose, plane, corner_directions(loose, rng), corner_directions(plane, rng)])
    rec[:, 32] = 1.0  # want_r2
    assert set(rec[:, 27]) == {0.0, 1.0, 2.0, 3.0} and len(rec) == 480
    if prec == F32:
        rec[:, 20:27] = K.f32r(rec[:, 20:27])
    got = gpu.kat(capi.KAT_SCAN_DISCS_XY, rec, prec)
    assert np.array_equal(got[:, 8:12], K.scan_pad_r2(rec, prec))
    r = rec.copy()
    r[:, 28:32] = got[:, 8:12]
    m = mirror_xy(xmirror, tmp_path, r, prec, capi.KAT_SCAN_DISCS_XY)
    same = bits(got[:, :8]) == bits(m)
    assert same.all(), (prec, np.flatnonzero(~same.all(1))[:8].tolist(), np.flatnonzero(~same.all(0)).tolist())
    # both branches of make_basis were there: the fallback e1 = (1, 0, 0) and the general one
    assert ((m[:, 6] == 1) & (m[:, 7] == 0)).sum() >= 60 and (m[:, 7] != 0).sum() >= 200
    # the XY forms are forms of their own: the XZ entry rounds differently on the same records
    assert not np.array_equal(bits(gpu.kat(capi.KAT_SCAN_DISCS, rec, prec)[:, :4]), bits(got[:, :4]))

    b = bucket_blocks(rng, 120)
    b = np.concatenate([b, corner_directions(b, rng)])
    if prec == F32:
        b[:, 20:27] = K.f32r(b[:, 20:27])
    got = gpu.kat(capi.KAT_BUCKET_DISCS_XY, b, prec)
    assert np.array_equal(got[:, 8:12], bucket_pad_r2(b, prec))
    r = b.copy()
    r[:, 28:32] = got[:, 8:12]
    m = mirror_xy(xmirror, tmp_path, r, prec, capi.KAT_BUCKET_DISCS_XY)
    same = bits(got[:, :8]) == bits(m)
    assert same.all(), (prec, np.flatnonzero(~same.all(1))[:8].tolist(), np.flatnonzero(~same.all(0)).tolist())
    disc, clear = f64_disc(b)  # conservative on the ray the kernel traces
    hit = (disc >= 0) & clear
    assert hit.sum() > 30 and (got[:, :4][hit] >= 0).all(), int((got[:, :4][hit] < 0).sum())
    with pytest.raises(capi.RayzHipError, match="v0"):
        bad = b[:4].copy()
        bad[1, 27] = np.inf
        gpu.kat(capi.KAT_BUCKET_DISCS_XY, bad, prec)
    with pytest.raises(capi.RayzHipError, match="class"):
        bad = rec[:4].copy()
        bad[2, 27] = 4.0
        gpu.kat(capi.KAT_SCAN_DISCS_XY, bad, prec)


# ---- 2. renders ------------------------------------------------------------------------------------------------------------------
W, H = 32, 18


def axis_camera(look_from, look_at, vup=(0, 1, 0)):
    return tracer.Tracer.init(W, 40.0, 10.0, 0.0, look_from, look_at, vup, seed=1).camera_desc()


def last_slot_scene():
    """A static run of exactly 64 whose LAST slot (the pool's last sphere: the run keeps pool order, and 64 leaves no pad behind it)
    is a sphere the camera sits on: every primary ray starts on its surface."""
    c, r = (0.5, 0.9, 6.0), 0.6
    s = Scene(51, look_from=(c[0], c[1] + r * 0.6, c[2] - r * 0.8), look_at=(0.0, 0.9, 0.0), width=W)
    s.group(0, 0.9, 63)
    s.tail.append((c, r, s.mats[0], (0.0, 0.0, 0.0)))
    return s.loose(n_static=2, n_movy=0, n_movg=0)


def _scene(name):
    """(scene, the form AUTO must choose); the scenes borrowed from the run and bucket tests are viewed through a 32-wide camera of
    their own view (VIEWS)."""
    if name == "run_of_64_and_3_loose":  # (the ground is the third)
        return Scene(52, width=W).group(0, 0.6, 64).loose(n_static=2, n_movy=0, n_movg=0), XY
    if name == "runs_65_71_72_73":
        s = Scene(53, width=W)
        for h, n in [(0.4, 65), (1.3, 71), (2.2, 72), (3.1, 73)]:
            s.group(0, h, n)
        return s.loose(), XY
    if name == "bucket_of_64_and_a_remainder":
        s = Scene(54, width=W)
        bucket_group(s, 0.8, 64, lambda: 0.3)
        bucket_group(s, 0.8, 10, lambda: s.rng.uniform(-0.9, -0.5))
        return s.loose(), XY
    if name == "two_runs_of_several_buckets":
        s, _ = _bucket_layout("two_runs")
        return s, XY
    if name == "row_in_a_static_run":  # more candidates in a 5-FMA loop than a lane parks
        s, _ = _layout("row_view")
        return s, XY
    if name == "row_in_a_bucket":
        s, _ = _bucket_layout("row_view")
        return s, XY
    if name == "camera_on_the_last_slot":
        return last_slot_scene(), XY
    if name == "loose_movy_outweighs_the_run":  # 64 plane slots against 72 loose y-moving ones: AUTO keeps XZ
        return Scene(55, width=W).group(0, 0.6, 64).loose(n_static=2, n_movy=70, n_movg=2), XZ
    raise KeyError(name)


VIEWS = {"row_in_a_static_run": ((-12.0, 1.0, 0.0), (10.0, 1.0, 0.0)), "row_in_a_bucket": ((-12.0, 1.0, 0.0), (10.0, 1.0, 0.0)),
         "two_runs_of_several_buckets": ((0.0, 7.0, 15.0), (0.0, 1.0, 0.0))}
SCENES = ["run_of_64_and_3_loose", "runs_65_71_72_73", "bucket_of_64_and_a_remainder", "two_runs_of_several_buckets",
          "row_in_a_static_run", "row_in_a_bucket", "camera_on_the_last_slot", "loose_movy_outweighs_the_run"]


def check_forms(gpu, oracle, xmirror, tmp_path, t, cams, auto_form, what):
    """One DeviceScene: AUTO's choice, then per precision and camera the frame under AUTO, XZ and XY == oracle mode B (segments
    too), and the BVH frame == the flat list's."""
    scene = t.scene_desc()
    lay = _run(xmirror, tmp_path, "form", _write(tmp_path, "s.bin", _spheres(t)))
    assert lay["form"] == auto_form, (what, lay)
    want = Want(oracle, scene)
    ds = gpu.DeviceScene(scene)
    try:
        assert ds.scan_form == auto_form, (what, ds.scan_form)  # before any render: a fact of the pool
        for prec in (F32, F64):
            for tag, cam in cams:
                p = params(t.params(), width=W, height=H, traversal=LINEAR, precision=prec)
                frames = []
                for form in (AUTO, XZ, XY):
                    ds.scan_form = form
                    assert ds.scan_form == (auto_form if form == AUTO else form)
                    got, st = render_checked(ds, want, cam, p, f"{what}, {tag}, precision {prec}, form {form}")
                    frames.append((got, st.segments))
                assert all(np.array_equal(f[0], frames[0][0]) and f[1] == frames[0][1] for f in frames), (what, tag, prec)
                ds.scan_form = AUTO
                pb = params(p, traversal=BVH)
                out = out_tensor(pb)
                ds.render_into(cam, pb, out.data_ptr())
                st = ds.sync()
                assert_images_equal(out.cpu().numpy(), frames[0][0], f"{what}, {tag}: BVH vs flat list, precision {prec}")
                assert st.segments == frames[0][1], (what, tag, prec)
    finally:
        ds.close()


@pytest.mark.parametrize("name", SCENES)
def test_scene_renders_alike_under_both_forms_and_like_the_oracle(gpu, oracle, xmirror, tmp_path, name):
    s, auto_form = _scene(name)
    t = s.build(spp=4, bounces=4)
    cam = axis_camera(*VIEWS[name]) if name in VIEWS else t.camera_desc()
    assert name in VIEWS or (t.params().width, t.params().height) == (W, H)
    check_forms(gpu, oracle, xmirror, tmp_path, t, [("own camera", cam)], auto_form, name)


def test_cameras_along_z_and_along_minus_y(gpu, oracle, xmirror, tmp_path):
    """Views exactly along +z (the XY basis's degenerate axis: h² = ud.x² + ud.y² smallest at the image centre) and exactly along −y
    (the XZ basis's), over a scene of static runs, buckets and loose spheres."""
    s = Scene(56, width=W).group(0, 0.5, 72).group(0, -1.0, 64)
    bucket_group(s, 1.2, 66, lambda: s.rng.uniform(0.20, 0.21))
    t = s.loose().build(spp=4, bounces=4)
    cams = [("along +z", axis_camera((0.0, 0.5, -16.0), (0.0, 0.5, 0.0), (0, 1, 0))),
            ("along -y", axis_camera((0.0, 18.0, 0.0), (0.0, 0.0, 0.0), (0, 0, -1)))]
    check_forms(gpu, oracle, xmirror, tmp_path, t, cams, XY, "axis cameras")


def test_repadded_device_scene_keeps_its_form(gpu, oracle, xmirror, tmp_path):
    """Near camera, a camera 20,000 units out (the larger origin bound re-pads the streams), near again: the form is the pool's, the
    frames the oracle's at every step."""
    s, _ = _scene("runs_65_71_72_73")
    t = s.build(spp=4, bounces=4)
    near = camera(oracle, ((0.0, 7.0, 15.0), 40.0, 10.0), W, H)
    far = camera(oracle, FAR, W, H)
    check_forms(gpu, oracle, xmirror, tmp_path, t, [("near", near), ("far", far), ("near again", near)], XY, "re-padded")
