"""Sparse renders without a device (rayz_hip_scene_render_pixels, `render.phase_sequence`, `render.lattice_pixels`; DESIGN.md
§4.21): the lattice helpers' bookkeeping, the refusals that are decided before a device is looked for, the numpy restatement of
the resolve against tests/noise_ref.py, and the Zig text."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import noise_ref
import sparse_ref
from rayz_amd import capi, render, tracer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("rayz_hip_scene_render_pixels", "rayz_hip_scene_render_pixels_f64")


# ---- the lattice helpers ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [2, 3, 4])
def test_phase_sequence_is_a_permutation_of_every_phase(f):
    seq = render.phase_sequence(f)
    assert len(seq) == f * f and sorted(seq) == [(px, py) for px in range(f) for py in range(f)]
    assert seq[0] == (0, 0)


def test_phase_sequence_refuses_other_factors():
    for f in (0, 1, 5):
        with pytest.raises(ValueError):
            render.phase_sequence(f)


@pytest.mark.parametrize("w,h,f", [(24, 24, 2), (24, 24, 3), (24, 24, 4), (20, 12, 2), (20, 12, 4)])
def test_lattice_pixels_orders_dest_and_union(w, h, f):
    seen = []
    for phase in render.phase_sequence(f):
        px, py = phase
        rows, rows_dest = (t.numpy() for t in render.lattice_pixels(w, h, f, phase, order="rows"))
        tiles, tiles_dest = (t.numpy() for t in render.lattice_pixels(w, h, f, phase, order="tiles"))
        assert rows.dtype == np.int32 and rows_dest.dtype == np.int32 and rows.shape == (w // f * (h // f),)
        # "rows" is the lattice frame row-major: its dest counts up
        assert rows_dest.tolist() == list(range(len(rows)))
        # both orders list the same set, each pixel once, with the same pixel -> dest map
        assert sorted(rows.tolist()) == sorted(tiles.tolist()) and len(set(rows.tolist())) == len(rows)
        assert dict(zip(rows.tolist(), rows_dest.tolist())) == dict(zip(tiles.tolist(), tiles_dest.tolist()))
        # dest inverts to the lattice frame: scattering the pixels' own coordinates by dest gives full[py::f, px::f]
        full = np.arange(w * h).reshape(h, w)
        for pixels, dest in ((rows, rows_dest), (tiles, tiles_dest)):
            frame = np.full((h // f) * (w // f), -1)
            frame[dest] = pixels
            assert np.array_equal(frame.reshape(h // f, w // f), full[py::f, px::f])
        # "tiles": the first 64 entries of a lattice frame with a whole tile are that 8x8 tile, row by row
        if w // f >= 8 and h // f >= 8:
            j, i = np.divmod(tiles_dest[:64], w // f)
            assert j.tolist() == [r for r in range(8) for _ in range(8)] and i.tolist() == list(range(8)) * 8
        seen += rows.tolist()
    assert sorted(seen) == list(range(w * h))  # the phases partition the frame


def test_lattice_pixels_refusals():
    for bad in (dict(width=25, height=24, f=2, phase=(0, 0)), dict(width=24, height=24, f=2, phase=(2, 0)),
                dict(width=24, height=24, f=2, phase=(0, -1)), dict(width=24, height=24, f=2, phase=(0, 0), order="zigzag")):
        with pytest.raises(ValueError):
            render.lattice_pixels(**bad)


def test_query_result_lattice_strides_every_field_present():
    g = render.QueryResult()
    g.index = torch.arange(12 * 8, dtype=torch.int32).reshape(8, 12)
    g.normal = torch.arange(12 * 8 * 3, dtype=torch.float32).reshape(8, 12, 3)
    lo = g.lattice(4, (3, 1))
    assert lo.index.is_contiguous() and torch.equal(lo.index, g.index[1::4, 3::4]) and tuple(lo.index.shape) == (2, 3)
    assert lo.normal.is_contiguous() and torch.equal(lo.normal, g.normal[1::4, 3::4])
    assert lo.point is None and lo.albedo is None and lo.is_chain is False
    with pytest.raises(ValueError):
        g.lattice(4, (4, 0))


# ---- refusals that need no device ------------------------------------------------------------------------------------------
def _scene(lib):
    t = tracer.threeSpheres(24, seed=1)
    t.samples_per_px = 12
    t.set_gpu(chunk_spp=4)
    h = C.c_void_p()
    assert lib.rayz_hip_scene_create(C.byref(t.scene_desc()), C.byref(h)) == capi.OK
    return t, h


def test_refusals_before_any_device(built):
    lib = capi.load()
    t, h = _scene(lib)
    cam, p = t.camera_desc(), t.params()
    px, out = C.c_void_p(1 << 20), C.c_void_p(2 << 20)  # never dereferenced: every call below returns before a device is looked for

    def call(fn=lib.rayz_hip_scene_render_pixels, scene=h, cam=cam, p=p, pixels=px, n=4, dest=None, dest_pixels=4, out=out, var=None):
        return fn(scene, C.byref(cam) if cam else None, C.byref(p) if p else None, pixels, n, dest, dest_pixels, out, var, None)

    try:
        assert call(scene=None) != capi.OK
        assert call(cam=None) == capi.ERR_BAD_ARG
        assert call(p=None) == capi.ERR_BAD_ARG
        assert call(pixels=None) == capi.ERR_BAD_ARG and b"list is null" in lib.rayz_hip_last_error()
        assert call(out=None) == capi.ERR_BAD_ARG and b"output pointer" in lib.rayz_hip_last_error()
        # dest_pixels: without d_dest it is n_pixels; with d_dest an output of no slots cannot hold an entry
        assert call(dest_pixels=5) == capi.ERR_BAD_ARG and b"dest_pixels" in lib.rayz_hip_last_error()
        assert call(dest_pixels=0) == capi.ERR_BAD_ARG
        assert call(dest=C.c_void_p(3 << 20), dest_pixels=0) == capi.ERR_BAD_ARG and b"0 pixels" in lib.rayz_hip_last_error()
        # the precision belongs to the entry
        p64 = capi.RenderParams.from_buffer_copy(bytes(p))
        p64.precision = capi.PRECISION_F64
        assert call(p=p64) == capi.ERR_BAD_ARG and b"precision" in lib.rayz_hip_last_error()
        assert call(fn=lib.rayz_hip_scene_render_pixels_f64) == capi.ERR_BAD_ARG and b"precision" in lib.rayz_hip_last_error()
        bad = capi.RenderParams.from_buffer_copy(bytes(p))
        bad.samples_per_px = 0
        assert call(p=bad) == capi.ERR_BAD_ARG
        # the oversized list: 2^31 entries, and 3 x 2^29 entries of three chunks each (the queue head is 32 bits)
        assert call(n=1 << 31, dest_pixels=1 << 31) == capi.ERR_BAD_ARG and b"work items" in lib.rayz_hip_last_error()
        assert call(n=3 << 29, dest_pixels=3 << 29) == capi.ERR_BAD_ARG and b"work items" in lib.rayz_hip_last_error()
        # an empty list is done before anything is looked at: no buffers, no device
        assert call(pixels=None, n=0, dest_pixels=0, out=None) == capi.OK
        assert call(pixels=None, n=0, dest=C.c_void_p(3 << 20), dest_pixels=7, out=None) == capi.OK
        assert call(n=0, dest_pixels=1) == capi.ERR_BAD_ARG
        if not torch.cuda.is_available():  # a valid request on a box without a GPU fails, it never computes
            assert call() == capi.ERR_NO_DEVICE
    finally:
        lib.rayz_hip_scene_destroy(h)


# ---- the resolve, restated ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("sizes", [[4, 4, 4], [16, 16, 8], [4], [64, 64, 32, 16, 16]], ids=lambda s: "x".join(map(str, s)))
def test_sparse_ref_is_noise_refs_fold_and_per_channel_variance(f64, sizes):
    rng = np.random.default_rng(5)
    K, n = len(sizes), 37
    sums = rng.uniform(0, 2, size=(K, n, 3)) * np.asarray(sizes, dtype=np.float64).reshape(K, 1, 1)
    sums[:, 3] = 0.0  # a black pixel
    sums[0, 5, 1] = np.nan
    sums[:, 7] = sums[0, 7]  # equal chunk sums of equal chunks: D rounds about zero, the clamp decides
    out, var = sparse_ref.resolve(sums, sizes, f64)
    M, Q = noise_ref.fold(sums, sizes, f64)
    N, R = sum(sizes), np.float64 if f64 else np.float32
    want = M.astype(R) * (R(1) / R(N))
    assert out.dtype == R and np.array_equal(out.view(np.uint64 if f64 else np.uint32), want.view(np.uint64 if f64 else np.uint32))
    # noise_ref.evaluate sums the channels' D: with the other two channels' state zeroed ((D + 0) + 0 = D) it is the channel's own
    for ch in range(3):
        keep = np.zeros(3)
        keep[ch] = 1.0
        v, _, _ = noise_ref.evaluate(np.where(keep, M, 0.0), np.where(keep, Q, 0.0), K, N)
        assert np.array_equal(var[:, ch].view(np.uint32), v.astype(np.float32).view(np.uint32)), ch
    assert np.isposinf(var).all() if K < 2 else (np.isfinite(var[np.arange(n) != 5]).all() and (var[3] == 0).all())


def test_sparse_ref_scatters_and_keeps_unnamed_slots():
    rng = np.random.default_rng(6)
    sums = rng.uniform(0, 1, size=(3, 5, 3))
    dest = np.array([9, 0, 4, 4, 2])
    out = np.full((11, 3), np.float32(-7))
    var = np.full((11, 3), np.float32(-9))
    sparse_ref.resolve(sums, [4, 4, 4], dest=dest, out=out, var=var)
    plain, plain_var = sparse_ref.resolve(sums, [4, 4, 4])
    untouched = np.setdiff1d(np.arange(11), dest)
    assert (out[untouched] == -7).all() and (var[untouched] == -9).all()
    for j in (0, 1, 4):
        assert np.array_equal(out[dest[j]], plain[j]) and np.array_equal(var[dest[j]], plain_var[j])
    assert any(np.array_equal(out[4], plain[j]) for j in (2, 3))  # one of the two entries that share a slot stays


# ---- the bindings' text ------------------------------------------------------------------------------------------------------
def test_zig_text_carries_the_sparse_prototypes():
    text = open(os.path.join(ROOT, "rayz_amd", "zig", "renderer_hip.zig")).read()
    text = "\n".join(re.sub(r"//.*$", "", l) for l in text.split("\n"))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "rayz_hip.h")).read(), flags=re.S)
    ztype = {"uint32_t": "u32", "float": "f32", "double": "f64", "RayzScene": "RayzScene", "RayzCameraDesc": "RayzCameraDesc",
             "RayzRenderParams": "RayzRenderParams"}
    for name in NEW:
        c = re.search(r"^int %s\(([^)]*)\);" % name, hdr, flags=re.M | re.S)
        z = re.search(r"pub extern fn %s\((.*?)\) c_int;" % name, text, flags=re.S)
        assert c and z, name
        cp = [re.match(r"^(const )?(\w+)(\*?) (\w+)$", " ".join(x.split())).groups() for x in c.group(1).split(",")]
        zp = [tuple(" ".join(x.split()).split(": ", 1)) for x in z.group(1).split(",") if x.strip()]
        assert len(cp) == len(zp) == 10
        for (const, ty, star, cname), (zname, zty) in zip(cp, zp):
            optional = cname.endswith("_or_null")
            assert zname == (cname[: -len("_or_null")] if optional else cname), (name, cname, zname)
            if ty == "void":
                assert zty == "?*anyopaque"
            elif not star:
                assert zty == ztype[ty]
            elif ty.startswith("Rayz"):
                assert zty == f"*{'const ' if const else ''}{ztype[ty]}"
            else:
                assert zty == f"{'?' if optional else ''}[*]{'const ' if const else ''}{ztype[ty]}", (name, cname, zty)
    assert {p[0] for p in capi.PROTOTYPES} >= set(NEW)
