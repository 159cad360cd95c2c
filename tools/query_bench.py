#!/usr/bin/env python3
"""Ray-query rates (rayz_hip_scene_query*) on configs 3 and 5: 1920x1080 camera rays (the G-buffer form) and 2·10^6 seeded
diffuse-bounce rays from their first hits, NEAREST and ANY, through the BVH and the flat list.  Mrays/s from the library's HIP
events around the query kernel (rayz_hip_query_sync: kernel_ms), median of --reps launches after a warm-up; next to it the
render's own BVH segment rate on the same scene (segments / kernel_ms of a low-spp render), the yardstick of DESIGN.md §4.10.
    python tools/query_bench.py [--reps 5] [--bounce 2000000] [--configs 3,5]
--chain: INSTEAD, the specular-chain G-buffer (rayz_hip_scene_query_camera_chain) on configs 2 and 3 at 1920x1080,
BVH and flat list: its kernel time beside the first-hit G-buffer's in the same process (both by the library's HIP events, median of
--reps after a warm-up), the mean segments per pixel and the depth histogram, for max_depth 2, 4 and 8 at the default max_fuzz.
    python tools/query_bench.py --chain [--reps 5]
--sampled: INSTEAD, the sampled G-buffer (rayz_hip_scene_query_camera_sampled) on configs 2 and 3 at 1920x1080, BVH
and flat list, n = 4 and 16 samples of 16 per pixel: its kernel time beside n times the first-hit G-buffer's — the two launches
alternating in one process, both by the library's HIP events, median of --reps pairs after a warm-up —, segments per second beside
the first-hit query's camera-ray rate, and, as context, the 16-spp render on the same scene: its kernel_ms and the share of it that
16 camera segments per pixel at the sampled query's rate would be.
    python tools/query_bench.py --sampled [--reps 5]"""
import argparse
import os
import statistics
import time
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rayz_amd import capi, render, tracer  # noqa: E402


def timed(fn, ds, reps):
    fn()
    ds.query_sync()
    ms = []
    for _ in range(reps):
        fn()
        ms.append(ds.query_sync().kernel_ms)
    return statistics.median(ms)


def bounce_rays(g, n, seed):
    """n diffuse-bounce rays: from first-hit points of the G-buffer (drawn with replacement), direction normal + a random unit
    vector (UNIT_SPHERE_SURFACE scatter), time uniform in [0, 1), tmax +inf."""
    gen = torch.Generator(device="cuda").manual_seed(seed)
    hit = (g.index >= 0).flatten().nonzero().flatten()
    pick = hit[torch.randint(0, len(hit), (n,), device="cuda", generator=gen)]
    pts = g.point.reshape(-1, 3)[pick].double()
    nrm = g.normal.reshape(-1, 3)[pick].double()
    u = torch.randn((n, 3), device="cuda", dtype=torch.float64, generator=gen)
    u = u / u.norm(dim=1, keepdim=True)
    d = nrm + u
    d[d.abs().sum(dim=1) == 0] = nrm[d.abs().sum(dim=1) == 0]
    t = torch.rand((n, 1), device="cuda", dtype=torch.float64, generator=gen)
    rays = torch.cat([pts, t, d, torch.full((n, 1), float("inf"), device="cuda", dtype=torch.float64)], dim=1)
    return rays.float().contiguous()


def render_segment_rate(t, spp=16):
    t.samples_per_px, t.max_bounces = spp, 50
    t.set_gpu(render_seed=1, traversal=capi.TRAVERSAL_BVH)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    out = torch.empty((p.height, p.width, 3), dtype=torch.float32, device="cuda")
    ds = render.DeviceScene(sd)
    torch.cuda.synchronize()
    ds.render_into(cam, p, out.data_ptr())
    ds.sync()
    ds.render_into(cam, p, out.data_ptr())
    st = ds.sync()
    ds.close()
    return st.segments / st.kernel_ms / 1e6  # Gsegments/s


def chain(args):
    scenes = {"2": lambda: tracer.randomBouncing(1920, seed=42), "3": lambda: tracer.randomBouncing(1920, -50, 50, seed=42)}
    for cfg, make in scenes.items():
        t = make()
        sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
        p.width, p.height, p.tmin = 1920, 1080, 1e-3
        ds = render.DeviceScene(sd)
        print(f"config {cfg}: {sd.n_spheres} spheres, 1920x1080", flush=True)
        for trav, tname in ((capi.TRAVERSAL_BVH, "bvh"), (capi.TRAVERSAL_LINEAR, "flat")):
            p.traversal = trav
            first = timed(lambda: ds.gbuffer(cam, p, outputs=render.QUERY_OUTPUTS), ds, args.reps)
            print(f"  {tname:4s} first-hit G-buffer {first:8.3f} ms", flush=True)
            for depth in (2, 4, 8):
                prm = dict(max_depth=depth, max_fuzz=capi.CHAIN_DEFAULTS["max_fuzz"])
                ms = timed(lambda: ds.gbuffer(cam, p, chain=prm), ds, args.reps)
                g = ds.gbuffer(cam, p, chain=prm)
                st = ds.query_sync()
                hist = torch.bincount(g.depth.flatten().long(), minlength=depth + 1).tolist()
                print(f"  {tname:4s} chain max_depth {depth}: {ms:8.3f} ms = x{ms / first:.2f} the first-hit G-buffer; "
                      f"{st.segments / st.primary_rays:.3f} segments per pixel; pixels by depth {hist}", flush=True)
        ds.close()


def sampled(args):
    scenes = {"2": lambda: tracer.randomBouncing(1920, seed=42), "3": lambda: tracer.randomBouncing(1920, -50, 50, seed=42)}
    spp, pixels = 16, 1920 * 1080
    for cfg, make in scenes.items():
        t = make()
        t.samples_per_px, t.max_bounces = spp, 50
        t.set_gpu(render_seed=1)
        sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
        p.width, p.height, p.tmin = 1920, 1080, 1e-3
        ds = render.DeviceScene(sd)
        out = torch.empty((1080, 1920, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        print(f"config {cfg}: {sd.n_spheres} spheres, 1920x1080, {spp} samples per pixel, camera with{'' if cam.defocus else 'out'} a defocus disk", flush=True)
        for trav, tname in ((capi.TRAVERSAL_BVH, "bvh"), (capi.TRAVERSAL_LINEAR, "flat")):
            p.traversal = trav
            ds.render_into(cam, p, out.data_ptr())  # (one run: context, timed by the library's events around the kernel alone)
            rs = ds.sync()
            for n in (4, 16):
                first, smp = [], []
                for k in range(args.reps + 1):  # (the first pair warms up)
                    ds.gbuffer(cam, p, outputs=("index", "t", "normal", "albedo"))
                    a = ds.query_sync().kernel_ms
                    ds.gbuffer_sampled(cam, p, samples=n)
                    st = ds.query_sync()
                    if k:
                        first.append(a)
                        smp.append(st.kernel_ms)
                f, s = statistics.median(first), statistics.median(smp)
                assert st.segments == pixels * n
                extra = f"; {st.node_tests / st.segments:.1f} box tests and {st.sphere_tests / st.segments:.2f} leaf tests per segment" if trav == capi.TRAVERSAL_BVH else ""
                print(f"  {tname:4s} n {n:2d}: sampled {s:8.3f} ms [{min(smp):.3f}, {max(smp):.3f}] = {pixels * n / s / 1e3:9.1f} Msegments/s; first-hit "
                      f"G-buffer {f:.3f} ms [{min(first):.3f}, {max(first):.3f}] = {pixels / f / 1e3:9.1f} Mrays/s, x {n} = {n * f:8.3f} ms; "
                      f"sampled / (n x first-hit) = {s / (n * f):.3f}{extra}", flush=True)
            print(f"  {tname:4s} render, {spp} spp, 50 bounces: kernel {rs.kernel_ms:.3f} ms, {rs.segments / rs.primary_rays:.2f} segments per path; "
                  f"its {spp} camera segments per pixel at the n = 16 sampled rate: {s:.3f} ms = {100 * s / rs.kernel_ms:.1f} % of it", flush=True)
        ds.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--bounce", type=int, default=2_000_000)
    ap.add_argument("--configs", default="3,5")
    ap.add_argument("--chain", action="store_true", help="the chain G-buffer beside the first-hit G-buffer instead")
    ap.add_argument("--sampled", action="store_true", help="the sampled G-buffer beside n first-hit G-buffers instead")
    args = ap.parse_args()
    render.init(0)
    if args.chain:
        return chain(args)
    if args.sampled:
        return sampled(args)
    scenes = {"3": lambda: tracer.randomBouncing(1920, -50, 50, seed=42), "5": lambda: tracer.triangleMesh(1920, 224, seed=1)}
    for cfg in args.configs.split(","):
        t = scenes[cfg]()
        sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
        p.width, p.height, p.tmin = 1920, 1080, 1e-3
        ds = render.DeviceScene(sd)
        p.traversal = capi.TRAVERSAL_BVH
        g = ds.gbuffer(cam, p)
        ds.query_sync()
        rays = bounce_rays(g, args.bounce, seed=7)
        occluded = ds.query(rays, kind="any")
        ds.query_sync()  # (the library's stream: wait before torch reads the result)
        print(f"config {cfg}: {sd.n_spheres} spheres, {sd.n_triangles} triangles; camera hit fraction "
              f"{float((g.index >= 0).float().mean()):.3f}; bounce hit fraction {float(occluded.hit.float().mean()):.3f}", flush=True)
        t0 = time.perf_counter()
        for _ in range(args.reps):
            ds.query(rays, kind="nearest", traversal=capi.TRAVERSAL_BVH)
            ds.query_sync()
        wall = (time.perf_counter() - t0) / args.reps * 1e3
        print(f"  bvh  bounce  NEAREST wall time per call, bound check and waits included: {wall:.3f} ms", flush=True)
        for trav, tname in ((capi.TRAVERSAL_BVH, "bvh"), (capi.TRAVERSAL_LINEAR, "flat")):
            p.traversal = trav
            ms = timed(lambda: ds.gbuffer(cam, p), ds, args.reps)
            print(f"  {tname:4s} camera  NEAREST (G-buffer) {1920 * 1080 / ms / 1e3:9.1f} Mrays/s  ({ms:.3f} ms)", flush=True)
            for kind in ("nearest", "any"):
                ms = timed(lambda: ds.query(rays, kind=kind, traversal=trav), ds, args.reps)
                st = ds.query_sync()
                extra = f"  {st.node_tests / st.segments:.1f} box tests/ray  {st.sphere_tests / st.segments:.2f} leaf tests/ray" if trav == capi.TRAVERSAL_BVH else ""
                print(f"  {tname:4s} bounce  {kind.upper():7s}            {len(rays) / ms / 1e3:9.1f} Mrays/s  ({ms:.3f} ms){extra}", flush=True)
        ds.close()
        print(f"  render (BVH, 16 spp, 50 bounces): {render_segment_rate(scenes[cfg]()):.2f} Gsegments/s", flush=True)


if __name__ == "__main__":
    main()
