"""Scenes that hand the flat list's OTHER two consumers — query_kernel<float / double> and the flat adaptive_pass_kernel, which
inline the scan text of trace_kernel_flat.hpp and always scan in the XZ basis without the set loop — every stream layout the form
kernels' own tests render: plane runs (tests/test_plane_runs_gpu.py: _layout), speed buckets (tests/test_speed_buckets_gpu.py:
_bucket_layout), one-radius sets (tests/test_one_radius_gpu.py: _scene; the XY scenes of tests/test_flat_xy_gpu.py reach here
through it) and the shortest scan loops (tests/test_scan_feed_gpu.py: _case).  The builders are used where they stand.
`check_layout()` asserts through the CPU mirrors' `layout` mode that a scene forms the runs, remainders, buckets, sets and slots it
was built for, and returns them as `units`: every run, remainder, bucket and set as the list of its members in slot order.
`query_rays()` makes each scene's ray batch: a ray_mix, and parts designed against that layout (see its docstring);
`check_designed_parts()` states on the reference's answers what each part was designed for."""
import numpy as np

from query_reference import TMIN, brute_force, narrow, pool_arrays, ray_mix
from rayz_amd import capi, tracer
from test_one_radius import check_layout as check_set_layout
from test_one_radius import set_sizes
from test_one_radius_gpu import _scene as _set_scene
from test_plane_runs import _run, _spheres, _write
from test_plane_runs_gpu import _layout as _run_layout
from test_plane_runs_gpu import assert_layout
from test_scan_feed_gpu import CASES as FEED_CASES
from test_scan_feed_gpu import _case as _feed_case
from test_scan_feed_gpu import assert_target_in_last_slot
from test_speed_buckets_gpu import _bucket_layout, assert_buckets

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
f32 = np.float32

RUNS = ["member_counts", "six_heights", "signed_zeros_and_negatives", "far_3e4", "f64_heights_one_f32", "row_view", "duplicates",
        "runs_only_and_loose_only", "loose_only_and_runs_only"]
BUCKETS = ["sizes_64_71_72_73", "mixed_sign", "two_runs", "far_3e4", "row_view", "wide_spread_no_bucket"]
SETS = ["sets_64_71_72_73_80", "two_radius_classes_in_one_bucket", "negative_radii", "camera_on_the_last_slot"]
NAMES = [f"runs.{n}" for n in RUNS] + [f"buckets.{n}" for n in BUCKETS] + [f"sets.{n}" for n in SETS] + [f"feed.{n}" for n in FEED_CASES]
QUERY_NAMES = list(NAMES)
ADAPTIVE_NAMES = ["runs.member_counts", "buckets.mixed_sign", "buckets.two_runs", "sets.sets_64_71_72_73_80", "buckets.row_view",
                  "runs.far_3e4"]
CAMERA_NAMES = ["runs.member_counts", "buckets.mixed_sign", "sets.sets_64_71_72_73_80"]
ROW_NAMES = ["runs.row_view", "buckets.row_view"]  # (tests/test_one_radius_gpu.py: row_in_a_static_set, row_in_a_bucket_set)
ROW_SETS = {"runs.row_view": [[96], []], "buckets.row_view": [[], [96]]}
MIX = 32  # rays ray_mix starts from (it returns about five times as many); cut from 384 to keep the GPU file's 92 tests short
SPP, BOUNCES = 8, 6  # of every scene's frame (the adaptive passes take 8 spp in chunks of 1)
# (look_from, look_at) where the builder's own view cannot meet a condition of the tests.  Through the builders' camera at
# (0, 7, 15) the median of these three scenes' noise estimates lies just under a power of 4, so that at the rel_error the adaptive
# test derives from it 0.76 to 0.88 of the pixels freeze before the end, above its 0.75; from here about 0.6 to 0.7 do.
CAMERAS = {"buckets.mixed_sign": ((0.0, 2.5, 10.0), (0.0, 1.0, 0.0)), "buckets.two_runs": ((9.0, 4.0, 10.0), (0.0, 1.0, 0.0)),
           "sets.sets_64_71_72_73_80": ((0.0, 2.0, 8.0), (0.0, 1.5, 0.0))}


def _build(name):
    """(tracer, what the family's builder says the scene must form)."""
    family, n = name.split(".", 1)
    if family == "runs":
        s, want = _run_layout(n)
        return s.build(spp=SPP, bounces=BOUNCES), want
    if family == "buckets":
        s, want = _bucket_layout(n)
        return s.build(spp=SPP, bounces=BOUNCES), want
    if family == "sets":
        s, want = _set_scene(n)
        return s.build(spp=SPP, bounces=BOUNCES), want
    if family == "feed":
        t, where = _feed_case(n)
        t.samples_per_px, t.max_bounces = SPP, BOUNCES
        return t, where
    raise KeyError(name)


def make(name):
    """A fresh tracer of the scene at the builder's own frame size (32x18 or 48x27), 8 spp, 6 bounces."""
    t = _build(name)[0]
    p = t.params()
    assert (p.width, p.height) in ((32, 18), (48, 27)) and (p.samples_per_px, p.max_bounces) == (SPP, BOUNCES)
    return t


def camera(name, t):
    """The scene's camera at its tracer's frame size: the builder's own, or the registry's (CAMERAS)."""
    if name not in CAMERAS:
        return t.camera_desc()
    return tracer.Tracer.init(t.params().width, 40.0, 10.0, 0.0, *CAMERAS[name], (0, 1, 0), seed=1).camera_desc()


# ---- the layout, by the library's own planner ----------------------------------------------------------------------------------
def check_layout(name, t, exes, tmp_path):
    """The layout `name` was built for, asserted as its family's own test asserts it (`exes`: the plane_filter, bucket and
    one_radius mirrors); then the properties every set layout has.  Returns {"units": [(kind, class, members in slot order)],
    "buckets": [(members, v0)], "in_runs": every sphere of a unit}: the units are every run, remainder, bucket and set, and the
    loose spheres of each class."""
    mirror, bmirror, omirror = exes
    family, n = name.split(".", 1)
    want = _build(name)[1]
    sph = _spheres(t)
    if family == "runs":
        assert_layout(mirror, tmp_path, t, want)
    elif family == "buckets":
        assert_buckets(mirror, bmirror, tmp_path, t, want)
    elif family == "feed":
        assert_target_in_last_slot(mirror, bmirror, tmp_path, t, want)
    lay = check_set_layout(mirror, bmirror, omirror, tmp_path, sph)
    if family == "sets":
        assert set_sizes(lay) == want, (name, set_sizes(lay))
        if n == "camera_on_the_last_slot":  # the sphere the camera sits on is the member in the set's last slot
            (run,), (st,) = lay["classes"][0]["runs"], lay["classes"][0]["sets"]
            assert st["end"] - run["first"] == 64 and run["order"][63] == len(sph) - 1
    if name in ROW_SETS:
        assert set_sizes(lay) == ROW_SETS[name], (name, set_sizes(lay))
    units, buckets = [], []
    for c, cl in enumerate(lay["classes"]):
        for r in cl["runs"]:
            order, f = r["order"], r["first"]
            units.append(("run", c, order))
            if c == 1:
                for b in r["buckets"]:
                    m = order[b["first"] - f:b["end"] - f]
                    units.append(("bucket", c, m))
                    buckets.append((m, float(np.uint32(b["v0_bits"]).view(f32))))
            rest = order[r["old_first"] - f:]  # what the run's own 4-field loop scans: no set or bucket took it
            if rest and len(rest) < len(order):
                units.append(("remainder", c, rest))
        for s in cl["sets"]:
            r = cl["runs"][s["run"]]
            units.append(("set", c, r["order"][s["first"] - r["first"]:s["end"] - r["first"]]))
    # the loose spheres of the three classes in stream order (pool order), without the oversized ground: the shortest loops of the
    # feed scenes are these
    loose = _run(mirror, tmp_path, "layout", _write(tmp_path, "s.bin", sph))["classes"]
    static = (sph[:, 3:6] == 0).all(1)
    movy = (sph[:, 3] == 0) & (sph[:, 5] == 0) & (sph[:, 4] != 0)
    for c, m in enumerate((loose[0]["loose"], loose[1]["loose"], np.flatnonzero(~static & ~movy).tolist())):
        m = [i for i in m if abs(sph[i, 6]) < 100]
        if m:
            units.append(("loose", c, m))
    for kind, c, m in units:
        assert len(m) >= 1 and len(set(m)) == len(m), (name, kind)
    in_runs = sorted({i for kind, _, m in units for i in m})
    return {"units": units, "buckets": buckets, "in_runs": in_runs}


# ---- rays for the query kernel --------------------------------------------------------------------------------------------------
def _rays(o, time, d, tmax=np.inf):
    n = len(o)
    return np.concatenate([o, np.broadcast_to(np.asarray(time, dtype=np.float64).reshape(-1, 1), (n, 1)), d,
                           np.broadcast_to(np.asarray(tmax, dtype=np.float64).reshape(-1, 1), (n, 1))], axis=1)


def _unit(a):
    a = np.asarray(a, dtype=np.float64)
    return a / np.linalg.norm(a, axis=-1, keepdims=True)


# where a member ray comes from, tried in this order (none from below: the ground is there)
DIRECTIONS = _unit([(0, 1, 0), (1, 1, 0), (-1, 1, 0), (0, 1, 1), (0, 1, -1), (1, 0.3, 1), (-1, 0.3, -1), (1, 0.2, -1)])
TIMES = np.array([0.0, 0.5, 1.0])


def duplicate_pairs(sd):
    """[(original, copy)] of spheres that are one sphere twice (centre, radius and velocity): copy > original in pool order."""
    c, v, r, _, _, _ = pool_arrays(sd)
    seen, out = {}, []
    for i in range(len(c)):
        key = (tuple(c[i]), tuple(v[i]), float(r[i]))
        if key in seen:
            out.append((seen[key], i))
        seen[key] = i
    return out


def member_rays(oracle, sd, ids, precision):
    """One ray per sphere of `ids`: the time cycles through 0, 0.5 and 1, the origin lies just outside the sphere where it is at
    that time, and the ray is aimed at its centre along the first of DIRECTIONS for which the mode-B brute force names that sphere
    the winner.  -> (rays, won): won[k] is False where no direction made ids[k] the winner (its ray then comes along the first)."""
    c, v, r, _, _, _ = pool_arrays(sd)
    ids = np.asarray(ids, dtype=np.int64)
    time = TIMES[np.arange(len(ids)) % 3]
    cen = c[ids] + v[ids] * time[:, None]
    rad = np.abs(r[ids])
    out = np.zeros((len(ids), 8))
    won = np.zeros(len(ids), dtype=bool)
    for k, u in enumerate(DIRECTIONS):
        todo = np.flatnonzero(~won)
        if not len(todo):
            break
        o = cen[todo] + u * (1.05 * rad[todo] + 0.01)[:, None]
        q = narrow(_rays(o, time[todo], np.broadcast_to(-u, (len(todo), 3))), precision)
        idx = brute_force(oracle, sd, q, TMIN, precision)[0]
        ok = idx == ids[todo]
        take = ok if k else np.ones(len(todo), dtype=bool)  # (the first direction stands where none wins)
        out[todo[take]] = q[take]
        won[todo[ok]] = True
    return out, won


def _edge_slots(m):
    """The members in the first and in the last group pair of a unit: the slots next to pad spheres and spare groups."""
    last = 8 * ((len(m) - 1) // 8)
    return list(m[:8]) + [i for i in m[last:] if i not in m[:8]]


RIM = 8


def rim_rays(sd, ids, origin, rng, spread):
    """RIM grazing rays per sphere of `ids`, as ray_mix makes them: from near `origin`, aimed at r·(1 − 1e-6), r and r·(1 + 1e-6) of
    the silhouette, twice each with tmax = inf; and two more that stop half-way (tmax = 0.5 of the way to the silhouette), so that a
    lane meets the slots next to the pads with a finite tbest that rejects them; times 0, 0.5, 1."""
    c, v, r, _, _, _ = pool_arrays(sd)
    k = np.repeat(np.asarray(ids, dtype=np.int64), RIM)
    m = len(k)
    tm = TIMES[np.arange(m) % 3]
    cen = c[k] + v[k] * tm[:, None]
    o = np.asarray(origin, dtype=np.float64)[None, :] + rng.normal(scale=spread, size=(m, 3))
    perp = np.cross(cen - o, rng.normal(size=(m, 3)))
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    target = cen + perp * (np.abs(r[k]) * (1 + np.tile([-1e-6, -1e-6, 0.0, 0.0, 1e-6, 1e-6, -1e-6, 0.0], len(ids))))[:, None]
    return _rays(o, tm, target - o, np.tile([np.inf] * 6 + [0.5, 0.5], len(ids)))


EDGE_FACTORS = (0.95, 1 - 1e-4, 1 - 1e-6, 1.0, 1 + 1e-6, 1 + 1e-4, 1.05)


def _pole_rays(c, v, r, i, rng):
    out = []
    for time in (0.0, 1.0):
        cen = c[i] + v[i] * time
        for pole in (1.0, -1.0):
            for _ in range(3):
                a = rng.uniform(0, 2 * np.pi)
                for fct in EDGE_FACTORS:
                    d = np.array([np.cos(a), pole * rng.uniform(-1e-3, 1e-3), np.sin(a)])
                    target = cen + np.array([0.0, pole * abs(r[i]) * fct, 0.0])
                    out.append(np.concatenate([target - d * rng.uniform(0.8, 2.0), [time], d * rng.choice([0.5, 1.0, 2.0]), [np.inf]]))
    return np.array(out)


def bucket_edge_rays(oracle, sd, buckets, rng, precision):
    """Per bucket, for the member whose speed is furthest from the bucket's v0 (where the term the bucket form leaves out,
    (vy − v0)·time·e2y, is largest against the padding h): near-horizontal rays that graze its top and bottom poles at times 0 and
    1, aimed at the pole's height times EDGE_FACTORS, from three sides and near by (its neighbours stand at its height).  A member
    whose poles lie buried in a neighbour can be hit by none of them (mode A): the member next in |vy − v0| is taken then, up to
    the eighth.  -> (rays, the member of each ray)."""
    c, v, r, _, _, _ = pool_arrays(sd)
    out, who = [], []
    for m, v0 in buckets:
        m = np.asarray(m)
        tries = []
        for i in m[np.argsort(-np.abs(v[m, 1] - v0), kind="stable")][:8]:
            q = narrow(_pole_rays(c, v, r, int(i), rng), precision)
            ia = brute_force(oracle, sd, q, TMIN, precision, mode="a")[0]
            tries.append((q, int(i)))
            if (ia == i).any() and (ia != i).any():
                break
        else:
            tries = tries[:1]
        out.append(tries[-1][0])
        who += [tries[-1][1]] * len(tries[-1][0])
    return (np.concatenate(out), np.array(who, dtype=np.int64)) if out else (np.zeros((0, 8)), np.zeros(0, dtype=np.int64))


ROW = 160  # rays of the `row` part: 64 with tmax = inf, 48 with tmax on a near root, 48 with tmax between the third sphere's roots


def _roots(sd, rays):
    """(near root, far root) in f64 of every (ray, sphere): nan where the discriminant is < 0."""
    c, v, r, _, _, _ = pool_arrays(sd)
    o, tm, d = rays[:, None, 0:3], rays[:, None, 3:4], rays[:, None, 4:7]
    q = c[None] + v[None] * tm - o
    a, hb = (d * d).sum(2), (d * q).sum(2)
    disc = hb * hb - a * ((q * q).sum(2) - r[None] ** 2)
    with np.errstate(invalid="ignore"):
        s = np.sqrt(disc)
    return (hb - s) / a, (hb + s) / a


def row_rays(sd, row, rng, precision):
    """ROW consecutive rays along the row of overlapping spheres `row` (one run, bucket or set): each passes through more than four
    of them, so a lane fills its four parking slots and flushes in mid-run.  The first 64 have tmax = inf; the next 48 have tmax on
    the near root of the 2nd, 4th and 6th sphere along the ray; the rest have tmax between the two roots of the 3rd: a finite tbest
    that rejects some parked candidates."""
    c, v, r, _, _, _ = pool_arrays(sd)
    row = np.asarray(row)
    x0 = c[row, 0].min() - 4.0
    time = TIMES[np.arange(ROW) % 3]
    y = c[row, 1].mean() + v[row, 1].mean() * time
    o = np.stack([np.full(ROW, x0), y + rng.uniform(-0.2, 0.2, ROW), rng.uniform(-0.15, 0.15, ROW)], axis=1)
    d = np.stack([np.ones(ROW), rng.uniform(-0.01, 0.01, ROW), rng.uniform(-0.01, 0.01, ROW)], axis=1)
    d = d * rng.choice([0.5, 1.0, 2.0], (ROW, 1))
    rays = narrow(_rays(o, time, d), precision)
    near, far = _roots(sd, rays)
    near = np.where(near >= TMIN, near, np.nan)
    order = np.argsort(near, axis=1)  # (nan last)
    pick = lambda a, k: a[np.arange(ROW), order[:, k]]  # noqa: E731
    for i in range(64, 112):
        rays[i, 7] = pick(near, (1, 3, 5)[i % 3])[i]
    for i in range(112, ROW):
        rays[i, 7] = 0.5 * (pick(near, 2)[i] + pick(far, 2)[i])
    assert np.isfinite(rays[64:, 7]).all()
    return narrow(rays, precision)


def candidates(sd, rays):
    """Per ray: how many spheres have an f64 discriminant >= 0, and how many of those have every root in [TMIN, inf) beyond the
    ray's tmax (candidates a finite tbest rejects)."""
    near, far = _roots(sd, rays)
    with np.errstate(invalid="ignore"):
        beyond = (np.where(near >= TMIN, near, far) > rays[:, 7:8]) & (far >= TMIN)
    return np.isfinite(near).sum(1), beyond.sum(1)


def query_rays(oracle, name, t, lay, precision, seed=0):
    """-> (rays (n, 8) float64 holding values of the precision, where).  `where` maps each part to its slice of the batch, and
    "far" to the slice of the rim rays that start 20,000 units out (they are last: the rest is the near batch); "member_ids",
    "rim_ids", "edge_ids" and "tie_ids" name the sphere each ray of those parts was made for.

    mix          query_reference.ray_mix, MIX camera rays and what it derives from them;
    members      one ray per sphere of a unit (run members and loose spheres) that some direction makes the winner (member_rays);
    rim          grazing rays at every member in the first and the last group pair of each run, remainder, bucket and set, from
                 near the scene's camera; rim_far: the same from 20,000 units out;
    bucket_edge  where a bucket has them (bucket_edge_rays);
    row          in the two row_view scenes (row_rays): the part starts on a multiple of 64, a wave takes 64 consecutive rays;
    ties         in `duplicates`: rays at the spheres that are in the pool twice, and the member rays no direction could win."""
    sd, cam = t.scene_desc(), camera(name, t)
    rng = np.random.default_rng([seed, sum(map(ord, name)), precision])
    c, v, r, _, _, _ = pool_arrays(sd)
    where, parts = {}, []
    if name in ROW_NAMES:
        row = max((m for kind, _, m in lay["units"] if kind == "run"), key=len)
        assert len(row) == 96
        parts.append(("row", row_rays(sd, row, rng, precision)))
    parts.append(("mix", ray_mix(oracle, t, precision, MIX, seed=sum(map(ord, name)) + 5)))
    ids = np.array(lay["in_runs"], dtype=np.int64)
    q, won = member_rays(oracle, sd, ids, precision)
    parts.append(("members", q[won]))
    where["member_ids"] = ids[won]
    pairs = duplicate_pairs(sd)
    if pairs or not won.all():
        tie = np.array([i for p in pairs for i in p], dtype=np.int64)
        lost = ids[~won]
        tq = [rim_rays(sd, tie, list(cam.look_from), rng, 0.5), member_rays(oracle, sd, tie, precision)[0]] if len(tie) else []
        parts.append(("ties", np.concatenate(tq + ([q[~won]] if len(lost) else []))))
        where["tie_ids"] = np.concatenate([np.repeat(tie, RIM), tie, lost])
    edge = sorted({i for _, _, m in lay["units"] for i in _edge_slots(m)})
    if lay["buckets"]:
        q, who = bucket_edge_rays(oracle, sd, lay["buckets"], rng, precision)
        parts.append(("bucket_edge", q))
        where["edge_ids"] = who
    if edge:
        parts.append(("rim", rim_rays(sd, edge, list(cam.look_from), rng, 0.5)))
        centre = c[edge].mean(axis=0)
        out = centre + 20000.0 * _unit(np.array(list(cam.look_from)) - centre)
        parts.append(("rim_far", rim_rays(sd, edge, out, rng, 50.0)))
        where["rim_ids"] = np.repeat(np.array(edge, dtype=np.int64), RIM)
    at = 0
    for k, p in parts:
        where[k] = slice(at, at + len(p))
        at += len(p)
    rays = narrow(np.concatenate([p for _, p in parts]), precision)
    where["far"] = where.get("rim_far", slice(len(rays), len(rays)))
    assert where["far"].stop == len(rays) and np.isfinite(rays[:, 0:7]).all() and (np.abs(rays[:, 4:7]).sum(axis=1) > 0).all()
    return rays, where


def check_designed_parts(name, sd, lay, rays, where, idx, oracle, precision):
    """What the designed parts of query_rays() were designed for, asserted on the reference's answers `idx` (mode B, brute force;
    a device's answers once they equal them).  Returns {"hit_share": of the whole batch}."""
    idx = np.asarray(idx, dtype=np.int64)
    c, v, r, _, _, _ = pool_arrays(sd)
    pairs = duplicate_pairs(sd)
    originals = {a for a, _ in pairs}
    assert bool(pairs) == (name == "runs.duplicates")
    if lay["in_runs"]:
        w = where["members"]
        ids = where["member_ids"]
        assert np.array_equal(idx[w], ids) and set(rays[w, 3]) == {0.0, 0.5, 1.0}
        # every run member that can win a ray at all does: only the first copy of a sphere that is there twice cannot
        assert set(lay["in_runs"]) - set(ids.tolist()) <= originals
        winners = set(ids.tolist())
        for kind, cls, m in lay["units"]:
            can = [i for i in m if i not in originals] if pairs else m
            assert can[0] in winners and can[-1] in winners, (name, kind, cls)
            if m[0] in originals or m[-1] in originals:  # (then its copy, the same sphere in a later slot, is the winner)
                assert all(dict(pairs)[i] in winners for i in (m[0], m[-1]) if i in originals)
            for g in range(0, len(m), 8):
                assert winners & set(m[g:g + 8]), (name, kind, cls, g)
        for part in ("rim", "rim_far"):
            w = where[part]
            at_target = (idx[w] == where["rim_ids"]).reshape(-1, RIM)
            assert w.stop - w.start == len(where["rim_ids"]) and at_target[:, :6].any(), (name, part)
            assert not at_target[:, 6:].any()  # (tmax half-way: whatever such a ray hits, it is nearer than its target)
        far_at_target = (idx[where["rim_far"]] == where["rim_ids"]).reshape(-1, RIM)[:, :6]
        assert not far_at_target.all()  # grazing: some touch what they aim at, some pass it
        assert (np.linalg.norm(rays[where["rim_far"], 0:3], axis=1) > 19000).all()
        assert (np.linalg.norm(rays[:where["far"].start, 0:3], axis=1) < 2000 + np.abs(c[:, 1]).max()).all()
        # the grazing rays do graze what they aim at (of those that start outside every sphere: one camera sits on a sphere)
        near, far = _roots(sd, rays[where["rim"]])
        with np.errstate(invalid="ignore"):
            outside = ~((near < 0) & (far > 0)).any(axis=1)
        outside &= np.isinf(rays[where["rim"], 7])  # (and of those that go all the way)
        assert outside.sum() >= 24 and (idx[where["rim"]] == where["rim_ids"])[outside].mean() > 0.25
    if lay["buckets"]:
        w = where["bucket_edge"]
        ia = brute_force(oracle, sd, rays[w], TMIN, precision, mode="a")[0]
        who = where["edge_ids"]
        per = len(who) // len(lay["buckets"])
        for k in range(len(lay["buckets"])):
            s = slice(k * per, (k + 1) * per)
            assert len(set(who[s])) == 1 and who[s][0] in lay["buckets"][k][0]
            assert (ia[s] == who[s]).any() and (ia[s] != who[s]).any(), (name, "bucket", k)
            assert set(rays[w][s, 3]) == {0.0, 1.0} and (np.abs(_unit(rays[w][s, 4:7])[:, 1]) <= 1.01e-3).all()
    else:
        assert "bucket_edge" not in where
    if name in ROW_NAMES:
        w = where["row"]
        assert w.start % 64 == 0 and w.stop - w.start == ROW >= 128
        n_cand, n_beyond = candidates(sd, rays[w])
        assert (n_cand > 4).all(), int(n_cand.min())
        tm = rays[w, 7]
        assert np.isinf(tm[:64]).all() and np.isfinite(tm[64:]).all()
        assert (n_beyond[64:] >= 1).any() and (idx[w][64:] >= 0).any()  # a finite tmax takes candidates away, and leaves winners
    else:
        assert "row" not in where
    if pairs:
        w = where["ties"]
        got, who = idx[w], where["tie_ids"]
        copy_of = dict(pairs)
        copies = set(copy_of.values())
        assert not (set(got.tolist()) & originals)  # the larger pool index wins every tie ..
        assert len(set(got.tolist()) & copies) >= len(pairs) // 2  # .. and the ties are there
        aimed_at_original = np.array([i in originals for i in who])
        hit_pair = np.array([g == copy_of.get(i, i) for g, i in zip(got, who)])
        assert hit_pair[aimed_at_original].sum() >= len(pairs)
    else:
        assert "ties" not in where
    share = float((idx >= 0).mean())
    assert 0.3 <= share <= 0.9, (name, share)
    return {"hit_share": share}


def without_ties(where, n):
    """The rays of the batch that the exact check takes: all but the `ties` part."""
    keep = np.ones(n, dtype=bool)
    if "ties" in where:
        keep[where["ties"]] = False
    return keep
