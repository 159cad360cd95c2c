"""Temporal accumulation's cubic resampling mode on the GPU (rayz_hip_temporal_set_resampling, `render.Temporal(resampling=...)`;
DESIGN.md §4.26): every colour, variance, length, W2 and taken byte of every step equals the CPU restatement
(tests/temporal_cubic_mirror.cpp) bit for bit — first, static, a fractional move and a further move, so the state a cubic step
leaves is read back — on the block fixture (where both the cubic and the fallback population are large), the plane, the general and
the moving sequence, plain and moments handles, defaults and binding parameters, with and without the taken bytes, in place for
the plain step; the mode switched on one handle; the hand-derived answers; the refusals of a live handle; a bilinear handle beside
a cubic one; and end to end on threeSpheres under an orbiting camera."""
import ctypes as C

import numpy as np
import pytest
import torch

import temporal_cases
import temporal_cubic_cases as cases
import temporal_cubic_f64
import temporal_cubic_ref as ref
from rayz_amd import capi, render, tracer

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (3, 3), (4, 4), (6, 5), (33, 9), (45, 23), (97, 41)]  # (4, 4): the smallest frame with one eligible window
ORIGINS = [(0, 0), (0, 0), (0.25, -0.625), (1.25, 0.375)]
BINDING = dict(alpha_min=0.4, n_max=20.0, normal_cos_min=0.99, max_rel_dist=0.02)


def same_bits(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    g, w_ = (got.view(np.uint32), want.view(np.uint32)) if got.dtype == np.float32 else (got, want)
    bad = np.argwhere(g != w_)
    assert len(bad) == 0, f"{what}: {len(bad)} of {got.size} values differ; first at {bad[:5].tolist()}: " \
                          f"{[(got[tuple(b)], want[tuple(b)]) for b in bad[:3]]}"


def camera_desc(cam):
    return capi.CameraDesc(**{k: tuple(float(x) for x in cam[k]) for k in ("look_from", "px_du", "px_dv", "px_origin")})


def to_gbuffer(index, normal, point):
    g = render.QueryResult()
    g.index, g.normal, g.point = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (index, normal, point))
    return g


def gpu_plain(tm, f, spp, in_place=False, **prm):
    x, v = torch.from_numpy(f["rgb"]).cuda(), torch.from_numpy(f["var"]).cuda()
    g = to_gbuffer(f["index"], f["normal"], f["point"])
    res = tm.step(x, v, g, camera_desc(f["camera"]), spp, out=x if in_place else None, var_out=v if in_place else None, length=True, **prm)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in res)


def gpu_moments(tm, f, spp, **prm):
    x = torch.from_numpy(f["rgb"]).cuda()
    g = to_gbuffer(f["index"], f["normal"], f["point"])
    res = tm.step_moments(x, g, camera_desc(f["camera"]), spp, length=True, w2=True, **prm)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in res)


def mirror_plain(m, f, spp, **prm):
    return m.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], spp, **prm)


def mirror_moments(m, f, spp, **prm):
    return m.step(f["rgb"], f["index"], f["normal"], f["point"], f["camera"], spp, **prm)


def run_sequence(frames, w, h, what, modes=None, **prm):
    """The frames through the mirrors and through device handles: a plain one with the taken bytes, a plain one in place without
    them, a moments one with them.  modes: the mode of each step (default: cubic throughout)."""
    modes = modes or ["cubic"] * len(frames)
    mp, mm = ref.Temporal(w, h), ref.TemporalMoments(w, h)
    a, b, c = render.Temporal(w, h), render.Temporal(w, h), render.Temporal(w, h, moments=True)
    ta, tc = torch.full((h, w), 77, dtype=torch.uint8, device="cuda"), torch.full((h, w), 77, dtype=torch.uint8, device="cuda")
    shares = []
    for k, (f, mode) in enumerate(zip(frames, modes)):
        spp = f.get("spp", 8)
        mp.resampling = mm.resampling = mode
        a.set_resampling(mode, taken=ta), b.set_resampling(mode), c.set_resampling(mode, taken=tc)
        assert a.resampling == b.resampling == c.resampling == mode and a.taken is ta and b.taken is None
        want = mirror_plain(mp, f, spp, **prm)
        for name, x, y in zip(("colour", "variance", "length"), gpu_plain(a, f, spp, **prm), want):
            same_bits(x, y, f"{what} step {k} ({mode}) {name}")
        same_bits(a.taken.cpu().numpy(), mp.taken, f"{what} step {k} ({mode}) taken")
        for name, x, y in zip(("colour", "variance", "length"), gpu_plain(b, f, spp, in_place=True, **prm), want):
            same_bits(x, y, f"{what} step {k} ({mode}) {name}, in place, no taken bytes")
        want = mirror_moments(mm, f, spp, **prm)
        for name, x, y in zip(("colour", "variance", "length", "W2"), gpu_moments(c, f, spp, **prm), want):
            same_bits(x, y, f"{what} moments step {k} ({mode}) {name}")
        same_bits(c.taken.cpu().numpy(), mm.taken, f"{what} moments step {k} ({mode}) taken")
        assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all()
        shares.append(float(mp.taken.mean()))
    a.close(), b.close(), c.close()
    return shares


@pytest.mark.parametrize("w,h", SIZES)
def test_device_equals_the_mirror_on_the_block_fixture(gpu, w, h):
    shares = run_sequence(cases.block_sequence(w, h, 11 * w + h), w, h, f"blocks {w}x{h}")
    assert shares[0] == shares[1] == 0  # a first frame and a static step take nothing
    if w >= 33:
        assert min(shares[2:]) > 0.15, shares  # (tests/test_temporal_cubic_cpu.py asserts the populations on the mirror)
    if h <= 3:
        assert max(shares) == 0  # height 3 is never eligible
    run_sequence(cases.block_sequence(w, h, 11 * w + h), w, h, f"blocks {w}x{h} binding", **BINDING)


@pytest.mark.parametrize("w,h", [(45, 23), (97, 41)])
def test_device_equals_the_mirror_on_the_other_sequences(gpu, w, h):
    run_sequence(temporal_cases.plane_sequence(w, h, 100 * w + h, ORIGINS), w, h, f"plane {w}x{h}")
    run_sequence(temporal_cases.general_sequence(w, h, 5 * w + h), w, h, f"general {w}x{h}")
    run_sequence(temporal_cases.moving_sequence(w, h, 3 * w + h), w, h, f"moving {w}x{h}")


def test_the_mode_switches_on_one_handle(gpu):
    """bilinear -> cubic -> bilinear -> cubic over the moved steps of one handle, each step equal to the mirror in that step's mode
    (the history a cubic step left is read by a bilinear one and back)."""
    w, h = 45, 23
    frames = cases.block_sequence(w, h, 5, shifts=((0.0, 0.0), (0.4, 0.3), (1.37, 0.61), (2.12, 1.43), (2.5, 2.0)))
    shares = run_sequence(frames, w, h, "switching", modes=["cubic", "bilinear", "cubic", "bilinear", "cubic"])
    assert shares[1] == shares[3] == 0 and shares[2] > 0.15 and shares[4] > 0.15


def test_device_gives_the_hand_derived_answers(gpu):
    def step(tm, s):
        f = dict(rgb=s.rgb, var=s.var, index=s.index, normal=s.normal, point=s.point, camera=s.camera)
        return gpu_plain(tm, f, s.spp, **s.params)

    for c in cases.cases() + [temporal_cubic_f64.length_case(), temporal_cubic_f64.variance_case()]:
        h, w = c.steps[0].index.shape
        tm = render.Temporal(w, h, resampling="cubic")
        tm.set_resampling("cubic", taken=True)
        rgb, var, length = c.run(tm, step)
        c.check(rgb, var, length, "device")
        c.check_taken(tm.taken.cpu().numpy(), "device")
        tm.close()
    for c in cases.bilinear_cases():
        h, w = c.steps[0].index.shape
        tm = render.Temporal(w, h)
        c.check(*c.run(tm, step), "device, bilinear")
        tm.close()

    def mstep(tm, s):
        f = dict(rgb=s.rgb, index=s.index, normal=s.normal, point=s.point, camera=s.camera)
        return gpu_moments(tm, f, s.spp, **s.params)

    for c in cases.moments_cases():
        h, w = c.steps[0].index.shape
        tm = render.Temporal(w, h, moments=True, resampling="cubic")
        c.check(*c.run(tm, mstep), "device")
        tm.close()


def test_refusals_on_a_live_handle(gpu):
    w, h = 8, 6
    f = cases.block_sequence(w, h, 3)[0]
    lib = capi.load()
    tm = render.Temporal(w, h, resampling="cubic")
    assert tm.resampling == "cubic" and tm.taken is None
    counts = torch.full((h, w), 8, dtype=torch.int32, device="cuda")
    x, v, g = torch.from_numpy(f["rgb"]).cuda(), torch.from_numpy(f["var"]).cuda(), to_gbuffer(f["index"], f["normal"], f["point"])
    with pytest.raises(ValueError, match="counts tensor"):
        tm.step(x, v, g, camera_desc(f["camera"]), counts)
    out, vout = torch.empty_like(x), torch.empty_like(v)
    prm, cam, o = capi.TemporalParams(**capi.TEMPORAL_DEFAULTS), camera_desc(f["camera"]), render._gbuffer_pointers(g, ["index", "normal", "point"])
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = lib.rayz_hip_temporal_step_counts(tm._h, C.byref(prm), C.byref(cam), ptr(counts), ptr(x), ptr(v), C.byref(o), ptr(out), ptr(vout), None, None)
    assert rc == capi.ERR_STATE and b"cubic" in lib.rayz_hip_last_error()
    assert lib.rayz_hip_temporal_set_resampling(tm._h, 2, None) == capi.ERR_BAD_ARG and tm.resampling == "cubic"
    with pytest.raises(ValueError, match="resampling must be"):
        tm.set_resampling("bicubic")
    # d_taken aliasing an output of the step
    taken = torch.zeros((h, w, 3, 4), dtype=torch.uint8, device="cuda")  # as large as a float32 frame
    assert lib.rayz_hip_temporal_set_resampling(tm._h, 1, ptr(taken)) == capi.OK
    for alias in ("out", "vout"):
        args = dict(out=ptr(out), vout=ptr(vout))
        args[alias] = ptr(taken)
        rc = lib.rayz_hip_temporal_step(tm._h, C.byref(prm), C.byref(cam), 8, ptr(x), ptr(v), C.byref(o), args["out"], args["vout"], None, None)
        assert rc == capi.ERR_BAD_ARG and b"d_taken" in lib.rayz_hip_last_error()
    rc = lib.rayz_hip_temporal_step(tm._h, C.byref(prm), C.byref(cam), 8, ptr(x), ptr(v), C.byref(o), ptr(out), ptr(vout), ptr(taken), None)
    assert rc == capi.ERR_BAD_ARG
    assert lib.rayz_hip_temporal_set_resampling(tm._h, 1, None) == capi.OK
    tm.close()
    # moments: counts and feedback
    tm = render.Temporal(w, h, moments=True, resampling="cubic")
    with pytest.raises(capi.RayzHipError, match="cubic"):
        tm.track_feedback()
    with pytest.raises(ValueError, match="counts tensor"):
        tm.step_moments(x, g, camera_desc(f["camera"]), counts)
    mprm = capi.TemporalMomentsParams(**capi.TEMPORAL_MOMENTS_DEFAULTS)
    rc = lib.rayz_hip_temporal_step_moments_counts(tm._h, C.byref(prm), C.byref(mprm), C.byref(cam), ptr(counts), ptr(x), C.byref(o), ptr(out),
                                                   ptr(vout), None, None, None)
    assert rc == capi.ERR_STATE and b"cubic" in lib.rayz_hip_last_error()
    # d_taken aliasing the moments step's length or W2 output
    plane = torch.zeros((h, w), dtype=torch.float32, device="cuda")
    assert lib.rayz_hip_temporal_set_resampling(tm._h, 1, ptr(plane)) == capi.OK
    for length, w2 in ((ptr(plane), None), (None, ptr(plane))):
        rc = lib.rayz_hip_temporal_step_moments(tm._h, C.byref(prm), C.byref(mprm), C.byref(cam), 8, ptr(x), C.byref(o), ptr(out), ptr(vout), length,
                                                w2, None)
        assert rc == capi.ERR_BAD_ARG and b"d_taken" in lib.rayz_hip_last_error()
    assert lib.rayz_hip_temporal_step_moments(tm._h, C.byref(prm), C.byref(mprm), C.byref(cam), 8, ptr(x), C.byref(o), ptr(out), ptr(vout), None,
                                              None, None) == capi.OK  # (the same call without the alias is taken)
    torch.cuda.synchronize()
    tm.reset()  # (that step left history, and a handle changes kind only without)
    tm.set_resampling("bilinear")
    tm.track_feedback()
    with pytest.raises(capi.RayzHipError, match="feedback"):
        tm.set_resampling("cubic")
    assert tm.resampling == "bilinear"
    tm.close()
    with pytest.raises(ValueError, match="feedback"):
        render.Temporal(w, h, moments=True, feedback=True, resampling="cubic")
    with pytest.raises(ValueError, match="resampling must be"):
        render.Temporal(w, h, resampling="cubik")


def test_a_replaced_taken_tensor_outlives_the_step_that_writes_it(gpu):
    """`set_resampling` directly behind an asynchronous step — dropping the taken tensor, or naming a new one — must not free the
    tensor that step is still writing: the step keeps it with its other tensors until the next step.  Checked by identity (the
    handle still refers to it) and by content (once the step has finished it holds the mirror's bytes), plain and moments."""
    w, h = 97, 41
    frames = cases.block_sequence(w, h, 13)
    for moments in (False, True):
        m = (ref.TemporalMoments if moments else ref.Temporal)(w, h, "cubic")
        tm = render.Temporal(w, h, moments=moments, resampling="cubic")
        for k, f in enumerate(frames):
            (mirror_moments if moments else mirror_plain)(m, f, 8)
            tm.set_resampling("cubic", taken=True)
            first = tm.taken
            x, v = torch.from_numpy(f["rgb"]).cuda(), torch.from_numpy(f["var"]).cuda()
            g = to_gbuffer(f["index"], f["normal"], f["point"])
            if moments:
                tm.step_moments(x, g, camera_desc(f["camera"]), 8)
            else:
                tm.step(x, v, g, camera_desc(f["camera"]), 8)
            if k % 2:
                tm.set_resampling("cubic")  # taken defaults to False: the handle names no tensor any more ..
                assert tm.taken is None
            else:
                tm.set_resampling("cubic", taken=True)  # .. or a new one
                assert tm.taken is not first
            assert any(t is first for t in tm._inflight), "the step that writes the tensor does not hold it"
            held = first.data_ptr()
            del first
            fresh = torch.full((h, w), 9, dtype=torch.uint8, device="cuda")  # (an allocation that could take a freed tensor's memory)
            assert fresh.data_ptr() != held
            torch.cuda.synchronize()
            same_bits(next(t for t in tm._inflight if isinstance(t, torch.Tensor) and t.data_ptr() == held).cpu().numpy(), m.taken,
                      f"{'moments' if moments else 'plain'} step {k}: the replaced taken tensor")
        assert m.taken.any()
        tm.close()


def test_a_bilinear_handle_beside_a_cubic_one_is_unchanged(gpu):
    """A default handle stepping between the steps of a cubic one gives what tests/temporal_ref.py's mirror of §4.15 gives."""
    import temporal_ref

    w, h = 45, 23
    frames = cases.block_sequence(w, h, 9)
    old = temporal_ref.Temporal(w, h)
    plain, cubic = render.Temporal(w, h), render.Temporal(w, h, resampling="cubic")
    assert plain.resampling == "bilinear"
    for k, f in enumerate(frames):
        gpu_plain(cubic, f, 8)
        want = old.step(f["rgb"], f["var"], f["index"], f["normal"], f["point"], f["camera"], 8)
        for name, x, y in zip(("colour", "variance", "length"), gpu_plain(plain, f, 8), want):
            same_bits(x, y, f"bilinear neighbour step {k} {name}")
    plain.close(), cubic.close()


def test_end_to_end_under_an_orbiting_camera(gpu, oracle):
    """threeSpheres at 64x36 under `orbit_views` (look_from AND look_at move), frames and first-hit G-buffers made on the device: a
    cubic handle equals the mirror fed the same device arrays, bit for bit; the taken share is printed."""
    t = tracer.threeSpheres(64, seed=3)
    t.samples_per_px, t.max_bounces = 8, 8
    t.set_gpu(render_seed=17, chunk_spp=0, traversal=capi.TRAVERSAL_BVH, tmin=1e-3)
    sd, p = t.scene_desc(), t.params()
    w, h = p.width, p.height
    ds = render.DeviceScene(sd)
    tm, m = render.Temporal(w, h, resampling="cubic"), ref.Temporal(w, h, "cubic")
    tm.set_resampling("cubic", taken=True)
    for k, view in enumerate(temporal_cases.orbit_views()):
        cam = temporal_cases.orbit_camera(oracle, view, w, h)
        q = capi.RenderParams.from_buffer_copy(p)
        q.seed = 40 + k
        frame = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ds.render_into(cam, q, frame.data_ptr())
        ds.sync()
        g = ds.gbuffer(cam, p)
        ds.query_sync()
        var = torch.full((h, w, 3), 0.01, device="cuda")
        out = tm.step(frame, var, g, cam, 8, length=True)
        torch.cuda.synchronize()
        want = m.step(frame.cpu().numpy(), var.cpu().numpy(), g.index.cpu().numpy(), g.normal.cpu().numpy(), g.point.cpu().numpy(), cam, 8)
        for name, x, y in zip(("colour", "variance", "length"), out, want):
            same_bits(x.cpu().numpy(), y, f"orbit frame {k} {name}")
        same_bits(tm.taken.cpu().numpy(), m.taken, f"orbit frame {k} taken")
        hit = g.index.cpu().numpy() >= 0
        print(f"orbit frame {k}: {m.taken[hit].mean():.3f} of the hit pixels took the cubic path, {(want[2][hit] > 8).mean():.3f} found history")
        if k >= 2:
            assert m.taken.any()
    tm.close(), ds.close()
