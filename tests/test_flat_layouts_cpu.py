"""The flat-list layouts of tests/flat_layout_scenes.py without a GPU: what rests on the scene and the oracle alone.  Every scene
forms the layout it was built for (by the library's own planner, through the three CPU mirrors' `layout`), and its ray batch does
what it was designed for on mode B's answers, which the query kernels must match bit for bit (tests/test_flat_layouts_gpu.py): the
winners cover every run, remainder, bucket and set (first slot, last real slot, a slot of every group of 8), every `row` ray has
more than four f64 candidates and a finite tmax takes some away, every bucket's edge rays both hit and miss per mode A, the hit
share of the batch lies in 0.3 – 0.9, and at least 0.8 of the batch without `ties` is unambiguous for the exact reference."""
import numpy as np
import pytest

import flat_layout_scenes as scenes
from query_exact import Scene, check_exact, exact_find_hit
from query_reference import TMIN, brute_force
from rayz_amd import capi
from test_one_radius import omirror  # noqa: F401  (a fixture)
from test_plane_runs import mirror  # noqa: F401  (a fixture)
from test_speed_buckets import bmirror  # noqa: F401  (a fixture)

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64


@pytest.mark.parametrize("name", scenes.NAMES)
def test_scene_forms_its_layout(built, mirror, bmirror, omirror, tmp_path, name):
    t = scenes.make(name)
    lay = scenes.check_layout(name, t, (mirror, bmirror, omirror), tmp_path)
    kinds = [k for k, _, _ in lay["units"]]
    family = name.split(".")[0]
    if family != "feed":
        assert "run" in kinds
    if family == "sets":
        assert "set" in kinds
    if family == "buckets":
        assert ("bucket" in kinds) == (name != "buckets.wide_spread_no_bucket")
    assert "loose" in kinds


def test_the_scenes_cover_every_unit_between_them(built, mirror, bmirror, omirror, tmp_path):
    """Runs of both classes and several per class, runs ending on and off whole group pairs, remainders behind buckets and behind
    sets, several buckets in one run, sets in runs and in buckets, a run with no bucket, and loose classes of 1 and of 2 spheres."""
    seen = set()
    for name in scenes.NAMES:
        lay = scenes.check_layout(name, scenes.make(name), (mirror, bmirror, omirror), tmp_path)
        per = {}
        for kind, c, m in lay["units"]:
            seen.add((kind, c))
            per[(kind, c)] = per.get((kind, c), 0) + 1
            if kind == "run":
                seen.add(("run ends on a group pair", len(m) % 8 == 0))
            if kind == "loose" and len(m) <= 2:
                seen.add(("short loose class", c))
        seen |= {("several", k) for k, n in per.items() if n > 1}
    want = {("run", 0), ("run", 1), ("bucket", 1), ("remainder", 0), ("remainder", 1), ("set", 0), ("set", 1), ("loose", 0), ("loose", 1),
            ("loose", 2), ("run ends on a group pair", True), ("run ends on a group pair", False), ("several", ("run", 0)),
            ("several", ("run", 1)), ("several", ("bucket", 1)), ("several", ("set", 0)), ("several", ("set", 1)), ("short loose class", 0),
            ("short loose class", 2)}
    assert want <= seen, want - seen


@pytest.mark.parametrize("prec", [F32, F64])
@pytest.mark.parametrize("name", scenes.QUERY_NAMES)
def test_query_ray_sets_do_what_they_were_designed_for(oracle, mirror, bmirror, omirror, tmp_path, name, prec):
    t = scenes.make(name)
    sd = t.scene_desc()
    lay = scenes.check_layout(name, t, (mirror, bmirror, omirror), tmp_path)
    rays, where = scenes.query_rays(oracle, name, t, lay, prec)
    idx, tt, rec, _ = brute_force(oracle, sd, rays, TMIN, prec)
    facts = scenes.check_designed_parts(name, sd, lay, rays, where, idx, oracle, prec)
    keep = scenes.without_ties(where, len(rays)) & (np.arange(len(rays)) < where["far"].start)
    S = Scene(sd)
    got = {"index": idx[keep], "t": tt[keep], "material": np.where(idx >= 0, S.mat[np.maximum(idx, 0)], -1)[keep], "point": rec[keep, 2:5],
           "normal": rec[keep, 5:8], "front_face": rec[keep, 8], "record": (idx < sd.n_spheres)[keep]}
    summary = check_exact(sd, rays[keep], got, exact_find_hit(sd, rays[keep], TMIN, prec, S), prec, S)
    print(name, prec, len(rays), "rays", facts, summary)
    assert summary["unambiguous"] >= 0.8
