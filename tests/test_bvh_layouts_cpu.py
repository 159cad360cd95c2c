"""The BVH layouts of tests/bvh_layout_scenes.py without a GPU: every scene forms the layout it was built for (by the library's own
builder, tests/bvh_layout_mirror.cpp); the oracle's mode B gives the same image and segments through its flat list and its BVH walk
on every one of them; and the scenes' query ray sets are mostly unambiguous for the exact reference (tests/query_exact.py), which is
the condition tests/test_bvh_layouts_gpu.py holds the query kernels under."""
import numpy as np
import pytest

import bvh_layout_scenes as scenes
from query_exact import Scene, check_exact, exact_find_hit
from query_reference import TMIN, brute_force
from rayz_amd import capi

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64


@pytest.fixture(scope="module")
def mirror(built, tmp_path_factory):
    return scenes.mirror_exe(str(tmp_path_factory.mktemp("bvh_layout")))


@pytest.mark.parametrize("name", scenes.NAMES)
def test_scene_forms_its_layout(mirror, tmp_path, name):
    sd = scenes.make(name).scene_desc()
    big = scenes.check_layout(name, sd, scenes.layout(mirror, sd, tmp_path / "scene.bin"))
    assert len(big) == len(scenes.PEELED[name])


def test_the_scenes_cover_every_layout_between_them(mirror, tmp_path):
    """A descriptor of two, several descriptors, a trailing descriptor of one, an oversized triangle, an oversized moving sphere,
    mixed descriptors both ways round, the cap of eight, the stop at kMinTree, and a tree at its depth budget."""
    seen = set()
    for name in scenes.NAMES:
        sd = scenes.make(name).scene_desc()
        e = scenes.layout(mirror, sd, tmp_path / "scene.bin")[(1, 1)]
        kinds = [scenes.kind_of(sd, i) for i in e["big"]]
        for d in e["descriptors"]:
            seen.add(("count", d["count"]))
            if d["count"] == 2:
                seen.add(("pair", tuple(d["triangle"])))
        seen.add(("descriptors", len(e["descriptors"])))
        seen |= {("kind", k) for k in kinds}
        if len(e["big"]) == e["max_big"] and e["in_tree"] + 8 == sd.n_spheres + sd.n_triangles:
            seen.add("cap")
        if e["big"] and e["in_tree"] == e["min_tree"]:
            seen.add("min_tree")
        if e["depth"] == e["budget"]:
            seen.add("budget")
    want = {("count", 1), ("count", 2), ("pair", (0, 0)), ("pair", (0, 1)), ("pair", (1, 0)), ("pair", (1, 1)), ("kind", "s"), ("kind", "m"),
            ("kind", "t"), "cap", "min_tree", "budget"} | {("descriptors", k) for k in range(5)}
    assert want <= seen, want - seen


@pytest.mark.parametrize("prec", [F32, F64])
@pytest.mark.parametrize("name", scenes.NAMES)
def test_mode_b_flat_list_equals_bvh(oracle, name, prec):
    t = scenes.make(name)
    t.set_gpu(precision=prec, traversal=capi.TRAVERSAL_LINEAR)
    sd, cam = t.scene_desc(), t.camera_desc()
    flat, sf = oracle.render_b(sd, cam, t.params())
    t.set_gpu(traversal=capi.TRAVERSAL_BVH)
    bvh, sb = oracle.render_b(sd, cam, t.params())
    assert flat.shape == (36, 64, 3) and flat.dtype == (np.float64 if prec == F64 else np.float32)
    assert np.array_equal(flat, bvh) and sf.segments == sb.segments and np.isfinite(flat).all()
    assert sf.segments > 1.1 * sf.primary_rays  # paths do bounce (walls0 and line600 are mostly sky)
    assert sf.node_tests == 0 and sb.node_tests > 0
    # light reaches the camera (the sky is the only source): the image can tell a lost or an invented hit
    assert (flat.sum(axis=2) > 0).mean() > 0.5 and len(np.unique(flat)) > 3000


@pytest.mark.parametrize("prec", [F32, F64])
@pytest.mark.parametrize("name", scenes.QUERY_NAMES)
def test_query_ray_sets_are_mostly_unambiguous_and_hit_what_they_aim_at(oracle, mirror, tmp_path, name, prec):
    """On mode B's answers (what the query kernels must match bit for bit): the exact reference accepts every ray's answer, at
    least 0.8 of each set is unambiguous, and the designed parts do what they were designed for."""
    t = scenes.make(name)
    sd = t.scene_desc()
    big = scenes.check_layout(name, sd, scenes.layout(mirror, sd, tmp_path / "scene.bin"))
    rays, where = scenes.query_rays(oracle, name, t, big, prec)
    S = Scene(sd)
    idx, tt, rec, _ = brute_force(oracle, sd, rays, TMIN, prec)
    got = {"index": idx, "t": tt, "material": np.where(idx >= 0, S.mat[np.maximum(idx, 0)], -1), "point": rec[:, 2:5],
           "normal": rec[:, 5:8], "front_face": rec[:, 8], "record": idx < sd.n_spheres}
    summary = check_exact(sd, rays, got, exact_find_hit(sd, rays, TMIN, prec, S), prec, S)
    print(name, prec, summary)
    assert summary["unambiguous"] >= 0.8
    scenes.check_designed_parts(name, sd, big, rays, where, idx, oracle, prec)
