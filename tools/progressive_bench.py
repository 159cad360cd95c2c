#!/usr/bin/env python3
"""Progressive rendering against the one-shot render on config 3 (randomBouncing a,b in [-50,50): 10,003 spheres,
1920x1080 x 1024 spp, 50 bounces, f32), through the BVH and the flat list, three ways:

  one-shot      rayz_hip_render_device: one trace launch over every chunk, then resolve_kernel
  1-chunk       rayz_hip_progressive_step(min_samples = 0): one launch per chunk of the schedule, each followed by the fold
  1/100         rayz_hip_progressive_step(min_samples = ceil(spp / 100)): passes of about 1/100 of the frame, whole chunks

Every form writes the frame (the progressive ones after every pass, as a viewer would) and must hash to the same bits.
Reported: whole-frame Msamples/s from host wall time (launches + the final wait), the trace kernels' summed time, the
time per pass, the trace time of every pass (a pass that starts at chunk 0 takes the kernel's uniform-prefix shortcut,
later ones read their chunk bounds from the table), and the peak chunk-sum workspace of each form.  Best of --reps.
"""
import argparse
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import ctypes as C  # noqa: E402

import torch  # noqa: E402

from rayz_amd import capi, render, tracer  # noqa: E402


def schedule(p):
    buf = (C.c_uint32 * 4096)()
    n = capi.load().rayz_hip_chunk_schedule(C.byref(p), buf, 4096)
    return list(buf[: n + 1])


def digest(out):
    return hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]


def one_shot(ds, cam, p, out):
    t0 = time.perf_counter()
    ds.render_into(cam, p, out.data_ptr())
    st = ds.sync()
    return time.perf_counter() - t0, st.kernel_ms, None


def progressive(ds, cam, p, out, min_samples):
    pr = ds.progressive(cam, p)
    try:
        t0 = time.perf_counter()
        windows = []
        while not pr.done:
            c0 = pr.chunks_done
            pr.step(min_samples, out.data_ptr())
            windows.append(pr.chunks_done - c0)
        st = pr.stats()  # waits for the last pass
        wall = time.perf_counter() - t0
        return wall, st.kernel_ms, windows
    finally:
        pr.close()


def pass_times(ds, cam, p, out):
    """Trace time of every one-chunk pass on its own (a wait after each)."""
    pr = ds.progressive(cam, p)
    ms, prev = [], 0.0
    try:
        while not pr.done:
            pr.step(0, out.data_ptr())
            k = pr.stats().kernel_ms
            ms.append(k - prev)
            prev = k
    finally:
        pr.close()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--grid", type=int, default=50)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--traversal", choices=["bvh", "linear", "both"], default="both")
    args = ap.parse_args()
    render.init(0)
    t = tracer.randomBouncing(args.width, -args.grid, args.grid, seed=42)
    t.samples_per_px = args.spp
    trav = {"bvh": [capi.TRAVERSAL_BVH], "linear": [capi.TRAVERSAL_LINEAR]}.get(args.traversal,
                                                                             [capi.TRAVERSAL_BVH, capi.TRAVERSAL_LINEAR])
    for tr in trav:
        t.set_gpu(render_seed=1, traversal=tr, precision=capi.PRECISION_F32, tmin=1e-3)
        scene, cam, p = t.scene_desc(), t.camera_desc(), t.params()
        sched = schedule(p)
        n = len(sched) - 1
        pixels = p.width * p.height
        samples = pixels * p.samples_per_px
        name = "bvh" if tr == capi.TRAVERSAL_BVH else "flat list"
        print(f"== config 3, {name}: {scene.n_spheres} spheres, {p.width}x{p.height} x {p.samples_per_px} spp, "
              f"{n} chunks {[b - a for a, b in zip(sched, sched[1:])]}", flush=True)
        out = torch.empty((p.height, p.width, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ds = render.DeviceScene(scene)
        try:
            forms = [("one-shot", lambda: one_shot(ds, cam, p, out)),
                     ("1-chunk", lambda: progressive(ds, cam, p, out, 0)),
                     ("1/100", lambda: progressive(ds, cam, p, out, (p.samples_per_px + 99) // 100))]
            one_shot(ds, cam, p, out)  # uploads, BVH build, workspace
            ref = digest(out)
            for label, run in forms:
                best = None
                for _ in range(args.reps):
                    out.fill_(float("nan"))
                    torch.cuda.synchronize()
                    wall, kms, windows = run()
                    if best is None or wall < best[0]:
                        best = (wall, kms, windows)
                    h = digest(out)
                    assert h == ref, (label, h, ref)
                wall, kms, windows = best
                passes = len(windows) if windows else 1
                peak = pixels * (max(windows) if windows else n) * 16
                acc = pixels * 16 if windows else 0
                print(f"  {label:9s} {samples / wall / 1e6:9.1f} Msamples/s (wall {wall * 1e3:8.1f} ms; trace kernels {kms:8.1f} ms, "
                      f"{samples / kms / 1e3:9.1f} Msamples/s) | {passes:3d} passes, {wall * 1e3 / passes:7.2f} ms per pass | "
                      f"chunk sums {peak / 1e6:7.1f} MB{f' + accumulator {acc / 1e6:.1f} MB' if acc else ''} | frame {h}",
                      flush=True)
            ms = pass_times(ds, cam, p, out)
            print("  trace ms per one-chunk pass (chunk size): " +
                  ", ".join(f"{m:.1f} ({b - a})" for m, a, b in zip(ms, sched, sched[1:])), flush=True)
        finally:
            ds.close()


if __name__ == "__main__":
    main()
