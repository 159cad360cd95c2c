"""Ray queries without a GPU: the C ABI refuses bad arguments before any HIP call, the brute-force reference the GPU tests
hold the query kernels to is itself held to hand-derived cases, and the query kernels' gfx950 code stays off its cliffs."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from rayz_amd import capi, tracer

from query_reference import brute_force

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _scene_handle(lib):
    t = tracer.threeSpheres(32, seed=1)
    sd = t.scene_desc()
    h = C.c_void_p()
    assert lib.rayz_hip_scene_create(C.byref(sd), C.byref(h)) == capi.OK
    return t, h


def test_query_arguments_are_checked_before_any_hip_call(built):
    lib = capi.load()
    t, h = _scene_handle(lib)
    out = capi.QueryOutputs()
    rays = C.c_void_p(0x1000)  # never dereferenced: every call below is refused (or is a no-op) before the device is touched
    try:
        def q(**kw):
            base = dict(n_rays=4, kind=capi.QUERY_NEAREST, precision=capi.PRECISION_F32, traversal=capi.TRAVERSAL_AUTO, tmin=1e-3)
            base.update(kw)
            return capi.QueryParams(**base)

        cases = [
            (None, C.byref(q()), rays, b"scene handle is null"),
            (h, None, rays, b"query params is null"),
            (h, C.byref(q()), None, b"rays is null"),
            (h, C.byref(q(kind=2)), rays, b"bad query kind 2"),
            (h, C.byref(q(precision=7)), rays, b"bad precision 7"),
            (h, C.byref(q(traversal=3)), rays, b"bad traversal 3"),
            (h, C.byref(q(tmin=float("nan"))), rays, b"tmin is NaN"),
        ]
        for scene, qp, r, msg in cases:
            assert lib.rayz_hip_scene_query(scene, qp, r, C.byref(out), None) == capi.ERR_BAD_ARG, msg
            assert msg in lib.rayz_hip_last_error(), (msg, lib.rayz_hip_last_error())
        assert lib.rayz_hip_scene_query(h, C.byref(q()), rays, None, None) == capi.ERR_BAD_ARG
        assert b"outputs is null" in lib.rayz_hip_last_error()
        # n_rays = 0 is defined as a no-op: OK, nothing launched (the scene is not even bound to a device)
        assert lib.rayz_hip_scene_query(h, C.byref(q(n_rays=0)), None, C.byref(out), None) == capi.OK
        # the camera form checks its params the same way
        cam, p = t.camera_desc(), t.params()
        assert lib.rayz_hip_scene_query_camera(None, C.byref(cam), C.byref(p), C.byref(out), None) == capi.ERR_BAD_ARG
        assert lib.rayz_hip_scene_query_camera(h, C.byref(cam), None, C.byref(out), None) == capi.ERR_BAD_ARG
        assert lib.rayz_hip_scene_query_camera(h, None, C.byref(p), C.byref(out), None) == capi.ERR_BAD_ARG
        assert b"camera is null" in lib.rayz_hip_last_error()
        p.traversal = 9
        assert lib.rayz_hip_scene_query_camera(h, C.byref(cam), C.byref(p), C.byref(out), None) == capi.ERR_BAD_ARG
        assert b"bad traversal 9" in lib.rayz_hip_last_error()
        p = t.params()
        p.shard_index, p.shard_count = 3, 3
        assert lib.rayz_hip_scene_query_camera(h, C.byref(cam), C.byref(p), C.byref(out), None) == capi.ERR_BAD_ARG
        # nothing queried yet: sync returns zero counters without a device
        st = capi.RenderStats(primary_rays=7)
        assert lib.rayz_hip_query_sync(h, C.byref(st)) == capi.OK and st.primary_rays == 0
        assert lib.rayz_hip_query_sync(None, None) == capi.ERR_BAD_ARG
    finally:
        lib.rayz_hip_scene_destroy(h)


def test_python_query_refuses_rays_outside_gpu_memory(built):
    """A host tensor never reaches the library (its pointer would be read by a kernel)."""
    import torch

    from rayz_amd import render

    t = tracer.threeSpheres(32, seed=1)
    ds = render.DeviceScene(t.scene_desc())
    try:
        with pytest.raises(ValueError, match="GPU memory"):
            ds.query(torch.zeros((4, 8), dtype=torch.float32))
        with pytest.raises(ValueError, match="GPU memory"):
            ds.query(np.zeros((4, 8), dtype=np.float32))
    finally:
        ds.close()


def _pool(spheres=(), triangles=()):
    """A SceneDesc of bare spheres (center, radius, velocity) and triangles (v0, v1, v2), one diffuse material."""
    tex = (capi.Texture * 1)(capi.Texture(kind=capi.TEX_SOLID, color=capi.D3(0.5, 0.5, 0.5)))
    mat = (capi.Material * 1)(capi.Material(kind=capi.MAT_DIFFUSE, texture=0, method=capi.DIFFUSE_HEMISPHERE))
    sph = (capi.Sphere * max(1, len(spheres)))(*[capi.Sphere(center=capi.D3(*c), velocity=capi.D3(*v), radius=r, material=0)
                                                for c, r, v in spheres])
    tri = (capi.Triangle * max(1, len(triangles)))(*[capi.Triangle(v0=capi.D3(*a), v1=capi.D3(*b), v2=capi.D3(*c), material=0)
                                                   for a, b, c in triangles])
    sd = capi.SceneDesc(spheres=sph, materials=mat, textures=tex, n_spheres=len(spheres), n_materials=1, n_textures=1,
                        n_triangles=len(triangles), triangles=tri)
    sd._keep = (tex, mat, sph, tri)
    return sd


def _ray(o, d, tmax=np.inf, time=0.0):
    return [o[0], o[1], o[2], time, d[0], d[1], d[2], tmax]


@pytest.mark.parametrize("precision", [capi.PRECISION_F32, capi.PRECISION_F64])
def test_brute_force_reference_on_hand_built_cases(oracle, precision):
    still = (0.0, 0.0, 0.0)
    # unit sphere at z = -5 seen from the origin along -z: roots exactly 4 and 6
    s0 = ((0.0, 0.0, -5.0), 1.0, still)
    sd = _pool([s0])
    rays = np.array([
        _ray((0, 0, 0), (0, 0, -1)),            # 0: nearest root 4
        _ray((0, 0, 0), (0, 0, -1), tmax=4.0),  # 1: tmax exactly on the root: inclusive
        _ray((0, 0, 0), (0, 0, -1), tmax=np.nextafter(4.0, 0.0) if precision else float(np.nextafter(np.float32(4), np.float32(0)))),  # 2: just below
        _ray((0, 0, -5), (0, 0, -1)),           # 3: origin inside: the far root, 1
        _ray((1, 0, 0), (0, 0, -1)),            # 4: tangent: the double root, 5
        _ray((0, 0, 0), (0, 0, 1)),             # 5: pointing away
    ])
    idx, t, rec, _ = brute_force(oracle, sd, rays, 1e-3, precision)
    assert idx.tolist() == [0, 0, -1, 0, 0, -1]
    assert t[0] == 4.0 and t[1] == 4.0 and t[3] == 1.0 and t[4] == 5.0 and np.isinf(t[2])
    assert rec[0, 2:5].tolist() == [0.0, 0.0, -4.0] and rec[0, 5:8].tolist() == [0.0, 0.0, 1.0] and rec[0, 8] == 1.0
    assert rec[3, 8] == 0.0 and rec[3, 5:8].tolist() == [0.0, 0.0, 1.0]  # from inside: the normal faces the ray, back face
    assert all(rec[k, 9] == 1.0 for k in (0, 1, 3, 4))  # the winners passed the reject filter
    # tmax between the roots with tmin past the near one: the far root (6) lies beyond tmax, a miss
    idx, t, _, _ = brute_force(oracle, sd, np.array([_ray((0, 0, 0), (0, 0, -1), tmax=5.0)]), 4.5, precision)
    assert idx.tolist() == [-1] and np.isinf(t[0])
    # .. and tmin below the near root with tmax between the roots: the near root
    idx, t, _, _ = brute_force(oracle, sd, np.array([_ray((0, 0, 0), (0, 0, -1), tmax=5.0)]), 1e-3, precision)
    assert idx.tolist() == [0] and t[0] == 4.0
    # two identical spheres: the later index wins the tie
    idx, t, _, _ = brute_force(oracle, _pool([s0, s0]), rays[:1], 1e-3, precision)
    assert idx.tolist() == [1] and t[0] == 4.0
    # nearest first over spheres and triangles: a triangle at z = -3 in front of the sphere, one at z = -4.5 behind its near root
    tri_near = ((-1.0, -1.0, -3.0), (1.0, -1.0, -3.0), (0.0, 1.0, -3.0))
    tri_far = ((-1.0, -1.0, -4.5), (1.0, -1.0, -4.5), (0.0, 1.0, -4.5))
    idx, t, _, _ = brute_force(oracle, _pool([s0], [tri_far, tri_near]), rays[:1], 1e-3, precision)
    assert idx.tolist() == [2] and t[0] == 3.0
    idx, t, _, _ = brute_force(oracle, _pool([s0], [tri_far]), rays[:1], 1e-3, precision)
    assert idx.tolist() == [0] and t[0] == 4.0
    # a triangle exactly at the sphere's near root: equal t, the larger index (the triangle) wins
    tri_tie = ((-1.0, -1.0, -4.0), (1.0, -1.0, -4.0), (0.0, 1.0, -4.0))
    idx, t, _, _ = brute_force(oracle, _pool([s0], [tri_tie]), rays[:1], 1e-3, precision)
    assert idx.tolist() == [1] and t[0] == 4.0


def _asm(tmp_path):
    from rayz_amd import _build

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    asm = tmp_path / "dev.s"
    flags = [f for f in _build.HIPFLAGS if f not in ("-fPIC", "-Wall", "-Wextra")]
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-o", str(asm), os.path.join(ROOT, "rayz_amd", "csrc", "rayz_hip.hip")],
                   check=True, capture_output=True, timeout=600)
    return asm.read_text()


def _bodies(text, pattern):
    out, name, body = {}, None, []
    for line in text.split("\n"):
        m = re.match(r"^(_ZN8rayz_dev\w*" + pattern + r"\w*):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
            elif not line.lstrip().startswith(";"):
                body.append(line)
    return out


def test_query_kernels_isa(tmp_path):
    """No VGPR spills and no scratch traffic in any query kernel; the BVH query kernels' box step keeps the node fetch's registers
    untouched while its loads are in flight (the check test_isa_invariants.py applies to the trace kernels)."""
    text = _asm(tmp_path)
    meta = {}
    for m in re.finditer(r"\.name:\s+(\S+)\n((?:\s+\.\w+:.*\n)+)", text):
        meta[m.group(1)] = dict(re.findall(r"\.(\w+):\s+(\S+)", m.group(2)))
    queries = {k: v for k, v in meta.items() if "query" in k}
    assert len(queries) == 8, sorted(queries)  # flat f32 / f64, BVH f32 / f64 x two record formats, bound check f32 / f64
    assert not any("trace_kernel" in k for k in queries)
    for name, f in queries.items():
        assert int(f["vgpr_spill_count"]) == 0, (name, f["vgpr_spill_count"])
        assert int(f["private_segment_fixed_size"]) == 0, (name, f["private_segment_fixed_size"])
    bodies = _bodies(text, "query")
    assert len(bodies) == 8, sorted(bodies)
    for name, L in bodies.items():
        assert not any(re.match(r"\s*scratch_(load|store)", l) for l in L), f"{name}: scratch traffic"
        assert not any(re.match(r"\s*flat_load", l) for l in L), f"{name}: a flat_load"
    blocks = 0
    for name, L in _bodies(text, "query_kernel_bvh").items():
        for i, line in enumerate(L):
            m = re.search(r"s_waitcnt vmcnt\((\d)\) lgkmcnt\((\d)\)", line)
            if not m or m.group(1) != m.group(2) or m.group(1) not in "12":
                continue
            n = int(m.group(1))
            dests, j = [], i - 1
            while j > 0 and i - j < 40:
                mm = re.search(r"(?:global_load_dwordx4|ds_read_b128) v\[(\d+):(\d+)\]", L[j])
                if mm:
                    dests.append((int(mm.group(1)), int(mm.group(2))))
                j -= 1
            assert len(dests) == 4 * n, (name, i, dests)
            regs = set()
            for a, b in dests[:n] + dests[2 * n:3 * n]:
                regs |= set(range(a, b + 1))
            k = i + 1
            while "s_waitcnt vmcnt(0) lgkmcnt(0)" not in L[k]:
                for a, b, c in re.findall(r"v\[(\d+):(\d+)\]|\bv(\d+)\b", L[k]):
                    used = {int(c)} if c else set(range(int(a), int(b) + 1))
                    assert not (used & regs), f"{name}: `{L[k].strip()}` touches a register of a node load still in flight"
                k += 1
                assert k - i < 80, (name, "no second wait after the split one")
            blocks += 1
    assert blocks >= 2 * 4  # two box steps per wave-level decision in each BVH query kernel
