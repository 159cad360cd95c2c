"""The feed of the flat list's scan loops (a running stream pointer, every scalar load issued right after a
wait, the furthest load one group behind the last pair) can only go wrong at a loop's ends, so the SHORTEST loops are rendered.
Member counts are taken per class, each with a backdrop of the other classes:
  * loose static spheres: 0, 1, 7, 8, 9, 16 (0: the loop is not entered; 1 and 7: one group pair, mostly pads; 9: two pairs);
  * a static plane run of 64, 65, 72 members (on and off whole group pairs, pads at the run's end);
  * a y-moving run of one 64-bucket whose 4-field remainder has 0, 1, 8 members (0: the run's own loop is skipped);
  * one speed bucket of 64 and one of 72;
  * spheres of general velocity: 0, 1, 3, 4 (groups of 2).
48x27 at 4 spp, 6 bounces.  Each frame is held bit for bit to oracle mode B (segments included) and to the device's BVH frame,
in f32 and f64 (tests/test_plane_runs_gpu.py: check_frames).  So that a loop that drops its last group cannot pass, the camera
looks at the sphere in the LAST slot of the loop under test (the last of the pool, which is the last of its class, run or
remainder; in a bucket, which is ordered by speed, the fastest), the layout mirrors confirm that slot, and the oracle's frame
must change when that sphere is taken out of the pool.  (Where the count is 0 there is no such sphere: the target is the last
sphere of the loop scanned next to the empty one.)"""
import numpy as np
import pytest

from helpers import assert_images_equal  # noqa: F401
from rayz_amd import capi
from test_plane_runs import _run, _spheres, _write, mirror  # noqa: F401  (mirror: a fixture)
from test_plane_runs_gpu import Scene, check_frames
from test_speed_buckets import bmirror, bucket_sizes, check_layout  # noqa: F401  (bmirror: a fixture)
from test_speed_buckets_gpu import bucket_group

pytestmark = pytest.mark.gpu

F32 = capi.PRECISION_F32
LINEAR = capi.TRAVERSAL_LINEAR
FROM = (0.0, 7.0, 15.0)
RUN_H = 0.9  # the height of the run under test


def _case(name, with_target=True):
    """(tracer, which loop holds the target: (kind, ...)) for a case name `<class>_<count>`.  The target is the last sphere added
    (Scene.tail: behind the shuffled pool), in front of the others as the camera sees them; with_target=False leaves it out and
    changes nothing else (the pool's other spheres, their order and the render seed are drawn before it)."""
    cls, n = name.rsplit("_", 1)
    n = int(n)
    seed = 700 + sum(map(ord, name))
    if cls == "static_loose":
        # the ground moves (1e-3 in y): the static class holds the n spheres below and nothing else
        pos = (0.0, 1.5, 10.0)
        s = Scene(seed, look_from=FROM, look_at=pos, ground_vy=1e-3)
        if n == 0:
            s.loose(n_static=0, n_movy=7, n_movg=6)
            target, where = (pos, 0.7, s.mats[0], (0.0, 0.3, 0.0)), ("movy_loose",)
        else:
            s.loose(n_static=n - 1, n_movy=8, n_movg=6)
            target, where = (pos, 0.7, s.mats[0], (0.0, 0.0, 0.0)), ("static_loose", n)
    elif cls == "static_run":
        pos = (0.0, RUN_H, 10.0)
        s = Scene(seed, look_from=FROM, look_at=pos).group(0, RUN_H, n - 1).loose()
        target, where = (pos, 0.45, s.mats[2], (0.0, 0.0, 0.0)), ("static_run", n)
    elif cls == "movy_remainder":
        pos = (0.0, RUN_H, 10.0)
        s = Scene(seed, look_from=FROM, look_at=pos)
        if n == 0:  # the bucket is the whole run; its fastest member is the target
            bucket_group(s, RUN_H, 63, lambda: 0.25)
            target, where = (pos, 0.45, s.mats[2], (0.0, 0.25 + 1e-4, 0.0)), ("bucket", 64, 0)
        else:  # 64 members of one speed, n of speeds far from it and from each other: no second bucket
            bucket_group(s, RUN_H, 64, lambda: 0.25)
            k = iter(range(n))
            bucket_group(s, RUN_H, n - 1, lambda: -0.5 + 0.05 * next(k))
            target, where = (pos, 0.45, s.mats[2], (0.0, -0.05, 0.0)), ("remainder", 64, n)
        s.loose()
    elif cls == "bucket":
        pos = (0.0, RUN_H, 10.0)
        s = Scene(seed, look_from=FROM, look_at=pos)
        bucket_group(s, RUN_H, n - 1, lambda: -0.3)
        s.loose()
        target, where = (pos, 0.45, s.mats[2], (0.0, -0.3 + 1e-4, 0.0)), ("bucket", n, 0)
    elif cls == "movg":
        pos = (0.0, 1.5, 10.0)
        s = Scene(seed, look_from=FROM, look_at=pos)
        if n == 0:
            s.loose(n_static=8, n_movy=7, n_movg=0)
            target, where = (pos, 0.7, s.mats[0], (0.0, 0.3, 0.0)), ("movy_loose",)
        else:
            s.loose(n_static=8, n_movy=8, n_movg=n - 1)
            target, where = (pos, 0.7, s.mats[0], (0.2, 0.1, -0.15)), ("movg", n)
    else:
        raise KeyError(name)
    if with_target:
        s.tail.append(target)
    return s.build(spp=4), where


CASES = ([f"static_loose_{n}" for n in (0, 1, 7, 8, 9, 16)] + [f"static_run_{n}" for n in (64, 65, 72)]
         + [f"movy_remainder_{n}" for n in (0, 1, 8)] + [f"bucket_{n}" for n in (64, 72)] + [f"movg_{n}" for n in (0, 1, 3, 4)])


def assert_target_in_last_slot(mirror, bmirror, tmp_path, t, where):
    """The scene forms the loop it was built for, and the pool's last sphere sits in that loop's last occupied slot."""
    sph = _spheres(t)
    last = len(sph) - 1
    lay = _run(mirror, tmp_path, "layout", _write(tmp_path, "s.bin", sph))["classes"]
    static = (sph[:, 3:6] == 0).all(1)
    movy = (sph[:, 3] == 0) & (sph[:, 5] == 0) & (sph[:, 4] != 0)
    kind = where[0]
    if kind == "static_loose":
        assert lay[0]["runs"] == [] and len(lay[0]["loose"]) == where[1] == static.sum() and lay[0]["loose"][-1] == last
    elif kind == "movy_loose":
        assert lay[1]["runs"] == [] and lay[1]["loose"][-1] == last
    elif kind == "static_run":
        (r,) = lay[0]["runs"]
        assert len(r["members"]) == where[1] and r["members"][-1] == last and r["first"] == 0
        assert r["end"] == -(-where[1] // 8) * 8
    elif kind == "movg":
        assert (~static & ~movy).sum() == where[1] and not static[last] and not movy[last]
    else:
        bl = check_layout(mirror, bmirror, tmp_path, sph)
        (r,) = bl["runs"]
        assert bucket_sizes(bl) == [[where[1]]], bucket_sizes(bl)
        if kind == "bucket":  # the bucket is the run: no remainder (the run's 4-field loop is skipped)
            assert r["bucketed"] == where[1] == len(r["order"]) == r["end"] - r["first"] and r["order"][where[1] - 1] == last
        else:  # the remainder: where[2] members behind the bucket, then pads to the whole group pair
            assert len(r["order"]) - r["bucketed"] == where[2] and r["order"][-1] == last
            assert r["end"] - r["first"] - r["bucketed"] == -(-where[2] // 8) * 8
    if kind not in ("static_loose", "movy_loose"):
        assert static.sum() - sum(len(r["members"]) for r in lay[0]["runs"]) >= 1  # (the other loops have work too)


@pytest.mark.parametrize("name", CASES)
def test_shortest_scan_loops_render_like_the_oracle(gpu, oracle, mirror, bmirror, tmp_path, name):
    t, where = _case(name)
    assert (t.params().width, t.params().height, t.samples_per_px, t.max_bounces) == (48, 27, 4, 6)
    assert_target_in_last_slot(mirror, bmirror, tmp_path, t, where)
    # not vacuous: the frame (mode B, on the CPU) needs the sphere in the loop's last slot
    t.set_gpu(traversal=LINEAR, precision=F32)
    want, _ = oracle.render_b(t.scene_desc(), t.camera_desc(), t.params())
    t0, _ = _case(name, with_target=False)
    t0.set_gpu(traversal=LINEAR, precision=F32)
    assert len(_spheres(t0)) == len(_spheres(t)) - 1 and t0.params().seed == t.params().seed
    without, _ = oracle.render_b(t0.scene_desc(), t0.camera_desc(), t0.params())
    assert not np.array_equal(want, without), f"{name}: the frame does not see the last slot's sphere (an error in this test)"
    check_frames(gpu, oracle, t, name)
