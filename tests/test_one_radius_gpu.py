"""One-radius sets (flat_one_radius_kernel: the XY kernel with the sets of a static plane run or a speed bucket scanned in blocks of
cx and cz against ONE padded r²) on the device: renders at the smallest scenes the set loop can go wrong at,
32x18 at 4 spp.  Each scene first asserts, through the mirror's `layout` (tests/one_radius_mirror.cpp), that it forms the sets it was
built for; then one DeviceScene is rendered with the form AUTO, XZ, XY and ONE_RADIUS, each frame held bit for bit to oracle mode B
(segments too) and the BVH frame to them; f32 and f64.  And the set form itself: RAYZ_KAT_SET_DISCS runs ScanGroup<float, 6>::discs
with the set's K1, K2 and padded R2 as scan_plane_class does, held bit for bit to the CPU mirror's `discs`, its R2 to the rule restated
here, and no member whose f64 discriminant is >= 0 is rejected."""
import subprocess

import numpy as np
import pytest

from helpers import assert_images_equal
from rayz_amd import capi
from test_flat_xy_gpu import H, VIEWS, W, axis_camera
import kat_records as K
from test_one_radius import bucket_h, omirror, set_sizes  # noqa: F401  (omirror: a fixture)
from test_plane_runs import _run, _spheres, _write
from test_plane_runs_gpu import Scene, _layout
from test_reuse_gpu import FAR, Want, camera, out_tensor, params, render_checked
from test_speed_buckets_gpu import _bucket_layout

pytestmark = pytest.mark.gpu

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
LINEAR, BVH = capi.TRAVERSAL_LINEAR, capi.TRAVERSAL_BVH
AUTO, XZ, XY, ONE = capi.SCAN_FORM_AUTO, capi.SCAN_FORM_XZ, capi.SCAN_FORM_XY, capi.SCAN_FORM_ONE_RADIUS


def members(s, cy, radii, vy=None, spread=8.0):
    """One sphere per radius at one height; vy() draws each speed (None: static)."""
    for r in radii:
        s.sphere((s.rng.uniform(-spread, spread), cy, s.rng.uniform(-spread, spread)), float(r), (0.0, float(vy()) if vy else 0.0, 0.0))
    return s


def last_slot_scene():
    """A static run of exactly 64 of one radius, one set: its LAST slot (the pool's last sphere: a set of one radius keeps pool
    order) is a sphere the camera sits on, so every primary ray starts on its surface."""
    c, r = (0.5, 0.9, 6.0), 0.6
    s = Scene(61, look_from=(c[0], c[1] + r * 0.6, c[2] - r * 0.8), look_at=(0.0, 0.9, 0.0), width=W)
    members(s, 0.9, [r] * 63)
    s.tail.append((c, r, s.mats[0], (0.0, 0.0, 0.0)))
    return s.loose(n_static=2, n_movy=0, n_movg=0)


def _scene(name):
    """(scene, [set sizes of the static class, of the mov-Y class])."""
    if name == "sets_64_71_72_73_80":  # leftovers of 0, 7, 8 and 9 members in the run's own loop, of 0 and 8 in the bucket's
        s = Scene(62, width=W)
        for h, n in [(0.4, 64), (1.3, 71), (2.2, 72), (3.1, 73)]:
            members(s, h, [0.3] * n)
        members(s, 0.8, [0.25] * 80, vy=lambda: 0.3)
        members(s, 1.7, [0.25] * 72, vy=lambda: -0.2)
        return s.loose(), [[64, 64, 64, 64], [80, 64]]
    if name == "radii_across_the_cap":  # one run: 65 at 0.32, 65 one step over 0.32·(1 + 1/16), 9 all apart
        s = Scene(63, width=W)
        members(s, 0.6, s.rng.permutation(np.concatenate([np.full(65, 0.32), np.full(65, 0.32 * (1 + 1 / 16) + 1e-9), 0.1 * 1.25 ** np.arange(9)])))
        return s.loose(), [[64, 64], []]
    if name == "radii_within_the_cap":  # .. and one step inside it: one set of both radii
        s = Scene(64, width=W)
        members(s, 0.6, s.rng.permutation(np.concatenate([np.full(65, 0.32), np.full(65, 0.32 * (1 + 1 / 16) - 1e-9)])))
        return s.loose(), [[128], []]
    if name == "two_radius_classes_in_one_bucket":
        s = Scene(65, width=W)
        members(s, 0.7, s.rng.permutation(np.concatenate([np.full(100, 0.2), np.full(100, 0.4)])), vy=lambda: s.rng.uniform(0.300, 0.305))
        return s.loose(), [[], [96, 96]]
    if name == "negative_radii":
        s = Scene(66, width=W)
        members(s, 0.5, [-0.3] * 70)
        members(s, 1.4, [-0.25] * 72, vy=lambda: s.rng.uniform(0.2, 0.21))
        return s.loose(), [[64], [64]]
    if name == "every_radius_differs":  # no set forms: ONE_RADIUS finds an empty set table and scans as XY does
        s = Scene(67, width=W)
        members(s, 0.6, 0.05 * 1.07 ** np.arange(40) * 1.0)
        members(s, 0.6, 0.05 * 1.07 ** (np.arange(40) + 0.5))
        return s.loose(), [[], []]
    if name == "row_in_a_static_set":  # more candidates inside a set than a lane parks
        s, _ = _layout("row_view")
        return s, [[96], []]
    if name == "row_in_a_bucket_set":
        s, _ = _bucket_layout("row_view")
        return s, [[], [96]]
    if name == "camera_on_the_last_slot":
        return last_slot_scene(), [[64], []]
    raise KeyError(name)


VIEW = {"row_in_a_static_set": VIEWS["row_in_a_static_run"], "row_in_a_bucket_set": VIEWS["row_in_a_bucket"]}
SCENES = ["sets_64_71_72_73_80", "radii_across_the_cap", "radii_within_the_cap", "two_radius_classes_in_one_bucket", "negative_radii",
          "every_radius_differs", "row_in_a_static_set", "row_in_a_bucket_set", "camera_on_the_last_slot"]


def check_forms(gpu, oracle, omirror, tmp_path, t, cams, want_sets, what, last_slot=None):
    """One DeviceScene: the sets it was built for, then per precision and camera the frame under AUTO, XZ, XY and ONE_RADIUS == oracle
    mode B (segments too), and the BVH frame == the flat list's."""
    scene = t.scene_desc()
    lay = _run(omirror, tmp_path, "layout", _write(tmp_path, "s.bin", _spheres(t)))
    assert set_sizes(lay) == want_sets, (what, set_sizes(lay))
    if last_slot is not None:  # the sphere the camera sits on is the member in the set's last slot
        (run,), (st,) = lay["classes"][0]["runs"], lay["classes"][0]["sets"]
        assert st["end"] - run["first"] == 64 and run["order"][63] == last_slot, (what, run["order"][60:])
    want = Want(oracle, scene)
    ds = gpu.DeviceScene(scene)
    try:
        assert ds.scan_form == XY, (what, ds.scan_form)  # AUTO: these sets hold fewer than 1,024 slots (test_auto_takes_the_set_kernel..); ONE forces them
        for prec in (F32, F64):
            for tag, cam in cams:
                p = params(t.params(), width=W, height=H, traversal=LINEAR, precision=prec)
                frames = []
                for form in (AUTO, XZ, XY, ONE):
                    ds.scan_form = form
                    assert ds.scan_form == (XY if form == AUTO else form)
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
def test_scene_renders_alike_under_every_form_and_like_the_oracle(gpu, oracle, omirror, tmp_path, name):
    s, want_sets = _scene(name)
    t = s.build(spp=4, bounces=4)
    cam = axis_camera(*VIEW[name]) if name in VIEW else t.camera_desc()
    assert name in VIEW or (t.params().width, t.params().height) == (W, H)
    last = len(_spheres(t)) - 1 if name == "camera_on_the_last_slot" else None  # (the tail sphere: the pool's last)
    check_forms(gpu, oracle, omirror, tmp_path, t, [("own camera", cam)], want_sets, name, last_slot=last)


def test_repadded_device_scene_keeps_its_sets(gpu, oracle, omirror, tmp_path):
    """Near camera, a camera 20,000 units out (the larger origin bound re-pads the streams and every set's R2), near again."""
    s, want_sets = _scene("sets_64_71_72_73_80")
    t = s.build(spp=4, bounces=4)
    near = camera(oracle, ((0.0, 7.0, 15.0), 40.0, 10.0), W, H)
    far = camera(oracle, FAR, W, H)
    check_forms(gpu, oracle, omirror, tmp_path, t, [("near", near), ("far", far), ("near again", near)], want_sets, "re-padded")


@pytest.mark.parametrize("n, form", [(1024, ONE), (1023, XY)])
def test_auto_takes_the_set_kernel_from_1024_set_slots(gpu, oracle, omirror, tmp_path, n, form):
    """plane_runs.hpp: kSetPayoffSlots.  A static run of n spheres of one radius: 1,024 of them in sets and AUTO reports and launches
    ONE_RADIUS; 1,023 leave 1,008 in sets and AUTO keeps XY.  Either way the frame is the oracle's."""
    s = Scene(70 + n % 2, width=W)
    members(s, 0.3, [0.12] * n, spread=12.0)
    t = s.loose().build(spp=4, bounces=4)
    lay = _run(omirror, tmp_path, "layout", _write(tmp_path, "s.bin", _spheres(t)))
    assert set_sizes(lay) == [[n // 16 * 16], []]
    scene, cam = t.scene_desc(), t.camera_desc()
    ds = gpu.DeviceScene(scene)
    try:
        assert ds.scan_form == form
        render_checked(ds, Want(oracle, scene), cam, params(t.params(), width=W, height=H, traversal=LINEAR, precision=F32), f"{n} one-radius members under AUTO")
        assert ds.scan_form == form
    finally:
        ds.close()


# ---- the set form ----------------------------------------------------------------------------------------------------------------
def set_blocks(rng, n):
    """RAYZ_KAT_SET_DISCS records and their members' radii: eight members at one height (small, negative, 3e4), half the records a
    static run's set, half a bucket's whose speeds lie up to r / 16 off v0; the one radius Rp = r·(1 + 1/16) with members' |radius| + h
    from Rp / (1 + 1/16) up to Rp itself; the ray aimed at member 0 where it is at the ray's time, near its rim for half the records."""
    rec = np.zeros((n, capi.KAT_IN_STRIDE))
    rec[:, 0:16] = K.f32r(rng.uniform(-9, 9, (n, 16)))
    rec[:, 16] = K.f32r(np.where(rng.random(n) < 0.25, 3.0e4, 0.0) + rng.uniform(-2, 3, n))
    movy = np.arange(n) % 2 == 1
    r = rng.uniform(0.2, 0.5, n)
    rec[:, 17] = np.where(movy, K.f32r(rng.uniform(-0.5, 0.5, n)), 0.0)
    rec[:, 18], rec[:, 19] = r * (1 + 1 / 16), movy
    vy = rec[:, 17:18] + (r / 16)[:, None] * rng.uniform(-1, 1, (n, 8)) * np.where(rng.random((n, 8)) < 0.3, 1.0, rng.random((n, 8)))
    rec[:, 28:36] = np.where(movy[:, None], vy, 0.0)
    h = np.where(movy[:, None], bucket_h(rec[:, 28:36], rec[:, 17:18]), 0.0)
    radius = (rec[:, 18:19] - h) * np.where(rng.random((n, 8)) < 0.3, 1.0, rng.uniform(1 / (1 + 1 / 16), 1.0, (n, 8))) * rng.choice([-1.0, 1.0], (n, 8))
    t = rng.random(n)
    rec[:, 26] = t
    tgt = np.stack([rec[:, 0], rec[:, 16] + rec[:, 28] * t, rec[:, 8]], 1)
    off = K.unit(rng.normal(size=(n, 3))) * (np.abs(radius[:, 0]) * np.where(rng.random(n) < 0.5, 1.0 + rng.uniform(-1e-4, 1e-4, n), rng.uniform(0, 2.0, n)))[:, None]
    o = tgt + rng.normal(size=(n, 3)) * rng.uniform(1, 30, (n, 1))
    rec[:, 20:23] = K.f32r(o)
    rec[:, 23:26] = K.f32r((tgt + off - rec[:, 20:23]) * rng.uniform(0.3, 3.0, (n, 1)))
    return rec, radius


def set_pad_r2(rec, precision):
    """rayz_hip.hip: pad_radius2_set, the largest over the record's eight members."""
    norm = lambda x, y, z: np.sqrt(x * x + y * y + z * z)  # noqa: E731
    vy, Rp = np.abs(rec[:, 28:36]), rec[:, 18:19]
    cn = norm(rec[:, 0:8], rec[:, 16:17], rec[:, 8:16]) + vy
    S = np.maximum(norm(rec[:, 20], rec[:, 21], rec[:, 22]), (cn + Rp).max(1))
    h = np.where(rec[:, 19:20] != 0, bucket_h(rec[:, 28:36], rec[:, 17:18]), 0.0)
    E = (32.0 if precision == F32 else 40.0) * 5.9604644775390625e-08 * (cn + h + Rp + S[:, None])
    v = (Rp + E) ** 2
    f = v.astype(np.float32)
    return np.where(f.astype(np.float64) < v, np.nextafter(f, np.float32(np.inf)), f).astype(np.float64).max(1)


@pytest.mark.parametrize("prec", [F32, F64])
def test_device_set_form(gpu, omirror, tmp_path, prec):
    rec, radius = set_blocks(np.random.default_rng(21), 40_000)
    if prec == F32:
        rec[:, 20:27] = K.f32r(rec[:, 20:27])
    got = gpu.kat(capi.KAT_SET_DISCS, rec, prec)
    assert np.array_equal(got[:, 10], set_pad_r2(rec, prec))
    r = rec.copy()
    r[:, 36] = got[:, 10]
    run = subprocess.run([omirror, "discs", str(_write(tmp_path, "rec.bin", r)), str(int(prec == F64))], capture_output=True, timeout=600)
    assert run.returncode == 0, run.stderr
    m = np.frombuffer(run.stdout, dtype=np.float32).reshape(-1, 10)
    bits = lambda x: np.asarray(x, dtype=np.float32).view(np.uint32)  # noqa: E731
    same = bits(got[:, :10]) == bits(m)
    assert same.all(), (prec, np.flatnonzero(~same.all(1))[:8].tolist(), np.flatnonzero(~same.all(0)).tolist())
    # conservative: every member's own sphere, where it is at the ray's time, on the ray the kernel traces
    o, d, t = rec[:, 20:23], rec[:, 23:26], rec[:, 26]
    hit = np.zeros((len(rec), 8), bool)
    for k in range(8):
        q = np.stack([rec[:, k] - o[:, 0], rec[:, 16] + rec[:, 28 + k] * t - o[:, 1], rec[:, 8 + k] - o[:, 2]], 1)
        a, hb, qq = (d * d).sum(1), (d * q).sum(1), (q * q).sum(1)
        disc = hb * hb - a * (qq - radius[:, k] ** 2)
        hit[:, k] = (disc >= 0) & (np.abs(disc) > 1e-11 * (hb * hb + a * (qq + radius[:, k] ** 2)))
    assert hit.sum() > 10_000 and (got[:, :8][hit] >= 0).all(), int((got[:, :8][hit] < 0).sum())
    assert 0.01 < (got[:, :8] >= 0).mean() < 0.5
    for at, bad, why in ((17, np.inf, "v0"), (18, -0.1, "Rp"), (19, 2.0, "movy")):
        with pytest.raises(capi.RayzHipError, match=why):
            b = rec[:4].copy()
            b[1, at] = bad
            gpu.kat(capi.KAT_SET_DISCS, b, prec)
