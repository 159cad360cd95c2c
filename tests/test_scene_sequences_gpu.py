"""One live `DeviceScene` through sequences of ray queries, camera, chain and sampled G-buffers, renders, sparse renders and
progressive steps, issued through the C ABI with no wait between them (scene_sequence.py): every output of every call equals the
answer of the same call on a fresh scene bit for bit, and the counters the two syncs report are the right call's.

The scene keeps state between calls — the stream of its last launch, the kind and traversal of the query in flight, the counters
buffer whose upper words the batch bound check uses, one device record of output pointers that chain and sampled calls rewrite
behind each other's kernels, the grow-only sums workspace, the render side's chunk sums, chunk table and counters, and the two
padded buffer sets with the BVH, rebuilt when a call needs a larger origin bound.  A stale flag, a record rewritten too early, a
counter left from the previous call or a workspace regrown under a queued kernel shows here as a wrong output or counter.
test_scene_sequences_cpu.py shows on the CPU that the scripts' frames, batches and lists hold the cases this relies on."""
import numpy as np
import pytest
import torch

import scene_sequence as sq
from rayz_amd import capi, render

pytestmark = pytest.mark.gpu

F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
BVH = capi.TRAVERSAL_BVH
N_HITTABLES = 6  # sampled_scenes' pool: a flat-list call tests each of them once per segment


@pytest.fixture(scope="module")
def ctx(oracle):
    return sq.context(oracle)


def allocate(ctx, calls):
    bufs = [sq.alloc(ctx, c) for c in calls]
    torch.cuda.synchronize()  # once, before the first library call
    return bufs


def queue(ds, ctx, calls, bufs):
    for c, b in zip(calls, bufs):
        sq.issue(ds, ctx, c, b)


def check_all(gpu, bufs, what):
    for k, b in enumerate(bufs):
        sq.check(gpu, b, f"{what}, call {k + 1}")


def check_stats(gpu, st, c, what, repadded=False):
    """`st` against the fresh scene's counters of `c`: rays and segments exactly; the tests exactly as well — the BVH walks of the
    query-side kernels deal their rays in fixed batches, so a repeated call repeats node_tests and sphere_tests (see
    test_bvh_counters_of_a_fresh_call_repeat) — but after a re-pad, where the wider filter may pass more candidates: only >=."""
    _, want = sq.expected(gpu, c)
    assert (st["primary_rays"], st["segments"]) == (want["primary_rays"], want["segments"]), (what, str(c), st, want)
    if c.traversal != BVH:
        assert st["node_tests"] == 0 and st["sphere_tests"] == st["segments"] * N_HITTABLES == want["sphere_tests"], (what, str(c), st, want)
    elif repadded:
        assert st["node_tests"] >= want["node_tests"] > 0 and st["sphere_tests"] >= want["sphere_tests"] > 0, (what, str(c), st, want)
    else:
        assert (st["node_tests"], st["sphere_tests"]) == (want["node_tests"], want["sphere_tests"]), (what, str(c), st, want)
        assert st["node_tests"] > 0 and st["sphere_tests"] > 0


def test_bvh_counters_of_a_fresh_call_repeat(gpu, ctx):
    """The premise of check_stats, observed on an MI355X: the same BVH call on two fresh scenes, and twice on one scene, reports the
    same node_tests and sphere_tests for every query-side kind in both precisions."""
    for c in [c for c in sq.one_stream() + sq.near_calls((BVH,)) if c.traversal == BVH]:
        _, want = sq.expected(gpu, c)
        ds = gpu.DeviceScene(ctx.scene)
        try:
            for k in range(2):
                (b,) = allocate(ctx, [c])
                sq.issue(ds, ctx, c, b)
                st = sq.query_sync(ds)
                assert st == want, (str(c), k, st, want)
        finally:
            ds.close()


# ---- 1. one stream, no sync between query-side calls ---------------------------------------------------------------------------------
def test_nine_queries_queued_on_one_stream(gpu, ctx):
    """Camera, chain, sampled (50x37), sampled f64 (the sums workspace grows while the call before is queued), a batch (its bound check
    blocks the host mid-queue and writes the counters' upper words), sampled n = 1, chain with other outputs and depth (the stores
    record rewritten), a batch, a sampled shard: one query_sync at the very end."""
    calls = sq.one_stream()
    ds = gpu.DeviceScene(ctx.scene)
    try:
        assert sq.query_sync(ds) == dict.fromkeys(sq.COUNTERS, 0)
        bufs = allocate(ctx, calls)
        queue(ds, ctx, calls, bufs)
        st = sq.query_sync(ds)
        again = sq.query_sync(ds)
        torch.cuda.synchronize()
        check_all(gpu, bufs, "unsynced")
        rows = render.shard_rows(ctx.params(calls[8]))
        assert rows == 16 and st["primary_rays"] == st["segments"] == rows * 64 * 5, st  # call 9's alone
        assert st["sphere_tests"] > 0 and st["node_tests"] == 0, st
        check_stats(gpu, st, calls[8], "the last call's counters")
        assert again == st
    finally:
        ds.close()


def test_nine_queries_each_followed_by_its_sync(gpu, ctx):
    """The same script with query_sync after every call: each call's counters are the fresh scene's for that call — a stale kind or
    traversal flag, counters left standing, or a chain call's kernel-counted segments leaking into the next call show here."""
    calls = sq.one_stream()
    ds = gpu.DeviceScene(ctx.scene)
    try:
        bufs = allocate(ctx, calls)
        for k, (c, b) in enumerate(zip(calls, bufs)):
            sq.issue(ds, ctx, c, b)
            st = sq.query_sync(ds)
            check_stats(gpu, st, c, f"call {k + 1}")
            assert sq.query_sync(ds) == st
        torch.cuda.synchronize()
        check_all(gpu, bufs, "synced")
    finally:
        ds.close()


def test_same_kind_back_to_back(gpu, ctx):
    """chain, chain, sampled, sampled with different outputs: each rewrites the one stores record behind a kernel of its own kind."""
    calls = sq.same_kind_back_to_back()
    ds = gpu.DeviceScene(ctx.scene)
    try:
        bufs = allocate(ctx, calls)
        queue(ds, ctx, calls, bufs)
        st = sq.query_sync(ds)
        torch.cuda.synchronize()
        check_all(gpu, bufs, "back to back")
        check_stats(gpu, st, calls[-1], "the last call's counters")
    finally:
        ds.close()


# ---- 2. three streams, no host sync ----------------------------------------------------------------------------------------------------
def test_six_queries_on_three_streams(gpu, ctx):
    """Each call is on another stream than the one before: the library waits for the scene's last launch itself; the stores record
    and the counters buffer are shared across the streams."""
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    streams = {0: 0, 1: s1.cuda_stream, 2: s2.cuda_stream}
    calls = [c.on(streams[k]) for c, k in sq.three_streams()]
    assert [c.stream != d.stream for c, d in zip(calls, calls[1:])] == [True] * 5
    ds = gpu.DeviceScene(ctx.scene)
    try:
        bufs = allocate(ctx, calls)
        queue(ds, ctx, calls, bufs)
        st = sq.query_sync(ds)
        torch.cuda.synchronize()
        check_all(gpu, bufs, "three streams")
        check_stats(gpu, st, calls[-1], "the last call's counters")
    finally:
        ds.close()


# ---- 3. queries among renders, sparse renders and progressive steps --------------------------------------------------------------------
@pytest.mark.parametrize("precision", [F32, F64], ids=["f32", "f64"])
def test_queries_among_renders_sparse_renders_and_steps(gpu, ctx, precision):
    ds = gpu.DeviceScene(ctx.scene)
    pr = None
    try:
        # render, sampled G-buffer with the render's params, sparse render of 300 listed pixels, chain G-buffer, render: one stream
        calls = sq.among_renders(precision)
        bufs = allocate(ctx, calls)
        queue(ds, ctx, calls, bufs)
        q = [sq.query_sync(ds)]
        r = [sq.counters(ds.sync()), sq.counters(ds.sync())]
        q += [sq.query_sync(ds), sq.query_sync(ds)]
        r.append(sq.counters(ds.sync()))
        torch.cuda.synchronize()
        check_all(gpu, bufs, "among renders")  # (expected() holds a fresh scene's frame to oracle mode B)
        assert q[0] == q[1] == q[2] and r[0] == r[1] == r[2], (q, r)
        check_stats(gpu, q[0], calls[3], "query_sync: the chain call's counters")
        check_stats(gpu, r[0], calls[4], "sync: the last render's counters")
        assert r[0]["segments"] != sq.expected(gpu, calls[0])[1]["segments"]  # (the two frames' counters differ: not the first's)
        px, dest, slots = ctx.pixels("s300")
        first = sq.host(bufs[0])["rgb"].reshape(-1, 3)
        sparse = sq.host(bufs[2])
        assert not sq.differences({"rgb": sparse["rgb"][dest]}, {"rgb": first[px]}), "the sparse slots are the first frame's pixels"
        unnamed = np.ones(slots, bool)
        unnamed[dest] = False
        assert np.isnan(sparse["rgb"][unnamed]).all() and np.isnan(sparse["var"][unnamed]).all() and int(unnamed.sum()) == slots - 300
        assert np.isnan(sparse["var"]).all() != (precision == F32)  # (asked for in f32 only)

        # a progressive handle of six chunks on the BVH, stepped half way; a sampled call in the other precision, a sparse render
        # with another chunk schedule and a chain call; then the rest of the handle
        hc = sq.handle_params(precision)
        between = sq.between_steps(precision)
        frame, more = allocate(ctx, [hc])[0], allocate(ctx, between)
        pr = ds.progressive(ctx.cameras[hc.cam], ctx.params(hc))
        assert pr.n_chunks == 6
        pr.step(3)
        queue(ds, ctx, between, more)
        assert pr.chunks_done == 3
        pr.step(sq.ALL, frame.out["rgb"].data_ptr())
        st = pr.stats()
        qs, rs = sq.query_sync(ds), sq.counters(ds.sync())
        torch.cuda.synchronize()
        assert pr.done
        check_all(gpu, more, "between a handle's steps")
        sq.check(gpu, frame, "the handle's frame is the one-shot frame (and the oracle's)")
        assert st.segments == sq.expected(gpu, hc)[1]["segments"] and st.primary_rays == 64 * 40 * 6  # (.. the oracle's: expected())
        check_stats(gpu, qs, between[2], "query_sync after the handle")
        check_stats(gpu, rs, between[1], "sync after the handle: the sparse render's counters")
    finally:
        if pr is not None:
            pr.close()
        ds.close()


# ---- 4. the origin bound grows in the middle of a queue --------------------------------------------------------------------------------
@pytest.mark.parametrize("node_format", [1, 2], ids=["bvh-planes", "bvh-indices"])
def test_the_origin_bound_grows_in_the_middle_of_a_queue(gpu, ctx, node_format):
    """Near calls, a batch 3,000 units out (the buffers the queued kernels read are rebuilt), the far camera's calls (rebuilt again,
    both precisions and the tree), the near calls again on the over-padded buffers — nothing waited for until the end."""
    sq.set_node_format(gpu, node_format)
    try:
        near, far_batch, far_cam, again = sq.growing_bound()
        calls = near + far_batch + far_cam + again
        ds = gpu.DeviceScene(ctx.scene)  # (the node format acts when the tree is built)
        try:
            bufs = allocate(ctx, calls)
            queue(ds, ctx, calls, bufs)
            st = sq.query_sync(ds)
            torch.cuda.synchronize()
            check_all(gpu, bufs, "a growing bound")
            check_stats(gpu, st, calls[-1], "the last call's counters", repadded=True)
            # .. and every near call once more with its own sync, for its counters
            more = allocate(ctx, again)
            for c, b in zip(again, more):
                sq.issue(ds, ctx, c, b)
                check_stats(gpu, sq.query_sync(ds), c, "near again", repadded=True)
            torch.cuda.synchronize()
            check_all(gpu, more, "near again, synced")
        finally:
            ds.close()
    finally:
        sq.set_node_format(gpu, 0)


# ---- 5. each kind as a scene's very first call; refusals with a call in flight ---------------------------------------------------------
@pytest.mark.parametrize("first", range(4), ids=["query", "camera", "chain", "sampled"])
def test_each_kind_as_the_first_call(gpu, ctx, first):
    """The counters buffer, the events and the stores record are allocated by whichever call comes first."""
    calls = sq.first_calls()
    calls = [calls[first]] + calls[:first] + calls[first + 1:]
    ds = gpu.DeviceScene(ctx.scene)
    try:
        assert sq.query_sync(ds) == dict.fromkeys(sq.COUNTERS, 0)
        bufs = allocate(ctx, calls)
        sq.issue(ds, ctx, calls[0], bufs[0])
        check_stats(gpu, sq.query_sync(ds), calls[0], "the first call")
        queue(ds, ctx, calls[1:], bufs[1:])
        st = sq.query_sync(ds)
        torch.cuda.synchronize()
        check_all(gpu, bufs, "first calls")
        check_stats(gpu, st, calls[-1], "the last call's counters")
    finally:
        ds.close()


def test_refusals_with_a_call_in_flight(gpu, ctx):
    """A sampled call is queued; then one call refused before any HIP call, one refused after its bound kernel ran on the stream and
    the host waited, and a sparse render with a pixel out of range.  The sampled call's counters and buffers are untouched, the
    refused calls wrote nothing, and the scene goes on."""
    in_flight, refused, accepted = sq.refusals()
    ds = gpu.DeviceScene(ctx.scene)
    try:
        bufs = allocate(ctx, [in_flight] + [c for c, _ in refused] + accepted)
        sq.issue(ds, ctx, in_flight, bufs[0])
        for (c, text), b in zip(refused, bufs[1:]):
            with pytest.raises(capi.RayzHipError, match=text):
                sq.issue(ds, ctx, c, b)
        st = sq.query_sync(ds)
        torch.cuda.synchronize()
        check_stats(gpu, st, in_flight, "the call in flight")
        sq.check(gpu, bufs[0], "the call in flight")
        for b in bufs[1:4]:
            sq.check_prefill(b, "a refused call")
        rest = bufs[4:]
        queue(ds, ctx, accepted, rest)
        qs, rs = sq.query_sync(ds), sq.counters(ds.sync())
        torch.cuda.synchronize()
        check_all(gpu, rest, "after the refusals")
        check_stats(gpu, qs, accepted[3], "query_sync after the refusals")
        check_stats(gpu, rs, accepted[4], "sync after the refusals")
        for b in bufs[1:4]:
            sq.check_prefill(b, "a refused call, later")
    finally:
        ds.close()
