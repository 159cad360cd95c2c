"""The scripts of scene_sequence.py show what test_scene_sequences_gpu.py claims for them — on the CPU, from the oracle and the
contracts' restatements (chain_ref, sampled_ref): chains that are followed and chains that are not, pixels some of whose samples
hit, both classes in every ray batch and in the far camera's frame, a sparse list with a duplicate whose `dest` leaves slots
unnamed, and a sums workspace that really grows in the middle of the first script."""
import numpy as np
import pytest

import chain_ref
import sampled_ref
import sampled_scenes as ss
import scene_sequence as sq
from rayz_amd import capi, render

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64


@pytest.fixture(scope="module")
def ctx(oracle):
    return sq.context(oracle)


def frame_pixels(p):
    return ss.shape_pixels(p.width, p.height, (p.shard_index, p.shard_count))


def test_the_scripts_name_every_kind_shape_and_camera():
    calls = sq.every_call()
    assert {c.kind for c in calls} == {"query", "camera", "chain", "sampled", "render", "sparse"}
    for kind in ("camera", "chain", "sampled"):
        mine = [c for c in calls if c.kind == kind]
        assert {c.precision for c in mine} == {F32, F64} and {c.traversal for c in mine} == {sq.LINEAR, sq.BVH}, kind
    shapes = {tuple(v for k, v in c.params if k in ("height", "shard_count", "shard_index", "width")) for c in calls if c.kind == "sampled"}
    assert shapes == {(40, 1, 0, 64), (37, 1, 0, 50), (40, 3, 1, 64)}
    assert {c.cam for c in calls if c.kind in ("chain", "sampled")} == {"lens", "pinhole", "far"}
    # the output subsets differ between neighbours of one kind (a stores record left as it was would show)
    a, b = [c for c in sq.one_stream() if c.kind == "chain"]
    assert set(a.outputs) != set(b.outputs) and a.arg("max_depth") != b.arg("max_depth")
    for x, y in zip(sq.same_kind_back_to_back()[::2], sq.same_kind_back_to_back()[1::2]):
        assert x.kind == y.kind and set(x.outputs) != set(y.outputs)


def test_chain_calls_follow_real_chains(ctx):
    """Every chain call's frame has pixels of depth > 0 and pixels of depth 0; every camera query's has hits and misses."""
    backends, done = {}, set()
    for c in sq.every_call():
        if c.kind not in ("chain", "camera") or c.key() in done:
            continue
        done.add(c.key())
        p = ctx.params(c)
        be = backends.setdefault(c.precision, chain_ref.OracleBackend(ctx.oracle, ctx.scene, c.precision))
        px, py = frame_pixels(p)
        r = chain_ref.chain(be, ctx.cameras[c.cam], px, py, ss.TMIN, c.arg("max_depth", 0), c.arg("max_fuzz", 0.25))
        hit = r["first_index"] >= 0
        assert 0 < int(hit.sum()) < len(px), (str(c), int(hit.sum()))
        if c.kind == "chain":
            assert int((r["depth"] > 0).sum()) > 0 and int((r["depth"] == 0).sum()) > 0, (str(c), np.bincount(r["depth"]).tolist())
            assert int(r["depth"].max()) <= c.arg("max_depth")


def test_sampled_calls_have_pixels_some_of_whose_samples_hit(ctx):
    """0 < hits < n somewhere in every sampled call of more than one sample; hits and misses in every one."""
    frames, done = {}, set()
    for c in sq.every_call():
        if c.kind != "sampled" or c.key() in done:
            continue
        done.add(c.key())
        p = ctx.params(c)
        n = c.arg("samples")
        assert 1 <= n <= p.samples_per_px
        key = (c.cam, c.precision, p.width, p.height, p.samples_per_px, p.seed)
        if key not in frames or frames[key]["index"].shape[1] < n:
            be = sampled_ref.OracleBackend(ctx.oracle, ctx.scene, c.precision)
            px, py = ss.shape_pixels(p.width, p.height)
            frames[key] = sampled_ref.records(be, ctx.oracle, ctx.cameras[c.cam], px, py, p.width, p.samples_per_px, p.seed, ss.TMIN, n=n)
        px, py = frame_pixels(p)
        hits = (frames[key]["index"][py * p.width + px, :n] >= 0).sum(axis=1)
        assert int((hits == 0).sum()) > 0 and int((hits == n).sum()) > 0, (str(c), np.bincount(hits).tolist())
        assert n == 1 or int(((hits > 0) & (hits < n)).sum()) > 0, (str(c), np.bincount(hits).tolist())


@pytest.mark.parametrize("precision", [F32, F64], ids=["f32", "f64"])
def test_every_batch_has_hits_and_misses(ctx, precision):
    import query_reference as qr

    sizes = {"r1000": 1000, "r257": 257, "far": 64}
    assert sizes["r257"] == 256 + 1
    for name, n in sizes.items():
        rays = ctx.rays(name, precision)
        assert rays.shape == (n, 8) and np.isfinite(rays[:, :7]).all()
        idx = qr.brute_force(ctx.oracle, ctx.scene, rays, ss.TMIN, precision)[0]
        assert int((idx >= 0).sum()) >= 8 and int((idx < 0).sum()) >= 7, (name, int((idx >= 0).sum()))
        assert len(set(idx[idx >= 0].tolist())) >= 3, (name, set(idx.tolist()))  # (not the ground alone)
    far = ctx.rays("far", precision)
    out = np.linalg.norm(far[:, 0:3], axis=1)
    assert (out > 2990).all() and (out < 3010).all()
    # beyond the padding a fresh scene starts with (the ground sphere: |c| + r = 2000), so the batch re-pads; the far camera again
    bound = max(np.linalg.norm(list(ctx.scene.spheres[i].center)) + ctx.scene.spheres[i].radius for i in range(ctx.scene.n_spheres))
    assert bound * 1.001 < out.min() and 2 * out.max() * 1.001 < np.linalg.norm(sq.FAR_FROM)
    bad = ctx.rays("nan1000", precision)
    assert np.isnan(bad[-1, 0]) and np.isfinite(bad[:-1, :7]).all() and np.isfinite(bad[-1, 1:7]).all()


def test_the_sparse_list_and_the_workspace(ctx):
    px, dest, slots = ctx.pixels("s300")
    assert len(px) == len(dest) == 300 and len(set(px.tolist())) < 300 and len(set(dest.tolist())) == 300  # duplicates in; slots once
    assert px.min() >= 0 and px.max() < sq.W * sq.H and dest.min() >= 0 and dest.max() < slots and slots - 300 > 0
    bad, none, _ = ctx.pixels("out of range")
    assert none is None and int((bad >= sq.W * sq.H).sum()) == 1 and int(bad.max()) == sq.W * sq.H
    # the sparse render between a handle's steps has another chunk schedule than the frames before it
    import ctypes as C

    def schedule(c):
        buf = (C.c_uint32 * 64)()
        p = ctx.params(c)
        return list(buf[: ctx.oracle.load().rayz_oracle_chunk_schedule(C.byref(p), buf, 64) + 1])

    first, other = sq.among_renders(F32)[2], sq.between_steps(F32)[1]
    assert first.kind == other.kind == "sparse" and schedule(first) != schedule(other) and len(schedule(other)) == 8
    assert len(schedule(sq.handle_params(F32))) == 7  # six chunks
    # the sums workspace (8 values of the precision per pixel, for calls of more than one sample) grows at the fourth call
    calls = sq.one_stream()
    need = []
    for c in calls:
        if c.kind == "sampled":
            p = ctx.params(c)
            need.append(render.shard_rows(p) * p.width * 8 * (8 if c.precision == F64 else 4) if c.arg("samples") > 1 else 0)
    assert need == [50 * 37 * 8 * 4, 64 * 40 * 8 * 8, 0, 16 * 64 * 8 * 4] and need[1] > need[0] > need[3]
    assert [c.kind for c in calls[2:4]] == ["sampled", "sampled"]  # .. while the third is still queued
