#!/usr/bin/env python3
"""The à-trous denoiser (rayz_hip_denoiser_*) on an MI355X: what a pass costs, against what, and what it buys.

1. Cost.  1920x1080 and 3840x2160, config 3's real G-buffer and a 16-spp frame.  Every launch of a run is bracketed by the handle's
   own HIP events (rayz_hip_denoiser_timing): the pack pass and each level, median [min, max] of --reps runs after --warmup.  Next
   to each level: a device-to-device copy, in the same process and timed with events the same way, that moves the level's
   COMPULSORY TRAFFIC — records read once (3 x 16 B per pixel) plus colour written once (16 B, or 12 B by the last level) = 64 or
   60 B per pixel, i.e. a copy of 32 or 30 B per pixel (read + write) — and the ratio level / copy.  The whole pass is also timed
   from outside (events on the caller's stream around the call: launches and their gaps included).  --paths repeats the level times
   with RAYZ_DEBUG_DENOISE_LDS_STRIDE = 0 (every level reads global memory) and 4 (LDS wherever the staged form exists): the
   per-stride comparison behind kDnLdsMaxStride (denoise.hpp).
2. Against what.  The 16-spp config-3 BVH frame the pass is meant to save re-rendering at more samples, timed in the same run
   (the library's trace-kernel events, rayz_hip_scene_sync, median of 9), next to the whole pass.
3. What it buys.  MSE of the noisy and the denoised 16-spp frame against a 1024-spp frame (--ref-spp), at 1920x1080.

    python tools/denoise_bench.py [--reps 100] [--warmup 10] [--ref-spp 1024] [--paths] [--sizes 1920,3840] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rayz_amd import capi, render, tracer  # noqa: E402


def event_ms(fn, stream, reps, warmup):
    """Median and (min, max) of `reps` event-bracketed calls of fn() on `stream`."""
    with torch.cuda.stream(stream):
        for _ in range(warmup):
            fn()
        stream.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def frame_and_gbuffer(width, spp, seed=1):
    t = tracer.randomBouncing(width, -50, 50, seed=42)  # config 3
    t.samples_per_px, t.max_bounces = spp, 50
    t.set_gpu(render_seed=seed, traversal=capi.TRAVERSAL_BVH)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    p.tmin = 1e-3
    ds = render.DeviceScene(sd)
    out = torch.empty((p.height, p.width, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ds.render_into(cam, p, out.data_ptr())
    ds.sync()
    ms = []
    for _ in range(9):
        ds.render_into(cam, p, out.data_ptr())
        ms.append(ds.sync().kernel_ms)
    g = ds.gbuffer(cam, p)
    ds.query_sync()
    return t, ds, cam, p, out, g, statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--paths", action="store_true")
    ap.add_argument("--sizes", default="1920,3840")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    render.init(0)
    stream = torch.cuda.Stream()
    result = {"levels": args.levels, "reps": args.reps, "sizes": {}}
    keep = None
    for width in (int(s) for s in args.sizes.split(",")):
        t, ds, cam, p, frame, g, frame_ms = frame_and_gbuffer(width, 16)
        w, h = p.width, p.height
        n = w * h
        dn = render.Denoiser(w, h)
        out = torch.empty_like(frame)
        src = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        dst = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        print(f"{w}x{h}: config 3 through the BVH at 16 spp: {frame_ms:.3f} ms (trace kernel, median of 9)", flush=True)
        size = {"frame_16spp_ms": frame_ms, "paths": {}}
        copies = {}
        for last in (False, True):
            nbytes = n * (30 if last else 32)  # read + written once = the level's 48 + 12 or 48 + 16 bytes per pixel of traffic
            copies[last] = event_ms(lambda: dst[:nbytes].copy_(src[:nbytes]), stream, args.reps, args.warmup)
            print(f"  copy moving a {'last' if last else 'middle'} level's compulsory traffic ({2 * nbytes / 1e6:.1f} MB read + written): "
                  f"{copies[last][0]:.4f} ms [{copies[last][1]:.4f}, {copies[last][2]:.4f}]  ({2 * nbytes / copies[last][0] / 1e9:.2f} TB/s)", flush=True)
        size["copy_mid_ms"], size["copy_last_ms"] = copies[False][0], copies[True][0]
        L = args.levels
        variants = [("default", -1)] + ([("direct", 0), ("lds", 4)] if args.paths else [])
        for vname, knob in variants:
            render.debug_set(capi.DEBUG_DENOISE_LDS_STRIDE, knob)
            fn = lambda: dn.run(frame, g, out=out, stream=stream.cuda_stream, levels=L)  # noqa: E731
            outside = event_ms(fn, stream, args.reps, args.warmup)
            packs, lv = [], [[] for _ in range(L)]
            with torch.cuda.stream(stream):
                for _ in range(args.reps):
                    fn()
                    pk, ms = dn.timing()
                    packs.append(pk)
                    for l in range(L):
                        lv[l].append(ms[l])
            render.debug_set(capi.DEBUG_DENOISE_LDS_STRIDE, -1)
            med = statistics.median
            rows = [{"what": "pack", "ms": med(packs), "min": min(packs), "max": max(packs)}]
            print(f"  [{vname:7s}] pack pass: {med(packs):.4f} ms [{min(packs):.4f}, {max(packs):.4f}]", flush=True)
            for l in range(L):
                cp = copies[l + 1 == L][0]
                m = med(lv[l])
                print(f"  [{vname:7s}] level {l} (stride {1 << l:2d}{', last' if l + 1 == L else ''}): {m:.4f} ms [{min(lv[l]):.4f}, {max(lv[l]):.4f}] = "
                      f"{m / cp:.2f} x the copy of its compulsory traffic", flush=True)
                rows.append({"what": f"level {l}", "stride": 1 << l, "ms": m, "min": min(lv[l]), "max": max(lv[l]), "ratio_to_copy": m / cp})
            kernels = med(packs) + sum(med(x) for x in lv)
            print(f"  [{vname:7s}] whole {L}-level pass: kernels {kernels:.4f} ms; from outside {outside[0]:.4f} ms [{outside[1]:.4f}, {outside[2]:.4f}]",
                  flush=True)
            size["paths"][vname] = {"rows": rows, "kernels_ms": kernels, "pass_ms": outside[0], "pass_min": outside[1], "pass_max": outside[2]}
        whole = size["paths"]["default"]["pass_ms"]
        size["pass_over_frame"] = whole / frame_ms
        verdict = "MORE than" if whole > frame_ms else "less than"
        print(f"  the whole {L}-level pass, {whole:.3f} ms, is {whole / frame_ms:.3f} x the 16-spp frame it filters: it costs {verdict} "
              f"that frame", flush=True)
        result["sizes"][f"{w}x{h}"] = size
        if width == 1920:
            keep = (t, ds, cam, p, frame.clone(), g, dn)
        else:
            dn.close()
            ds.close()
    if keep is not None and args.ref_spp:
        t, ds, cam, p, noisy, g, dn = keep
        p.samples_per_px = args.ref_spp
        ref = torch.empty_like(noisy)
        torch.cuda.synchronize()
        ds.render_into(cam, p, ref.data_ptr())
        st = ds.sync()
        den = dn.run(noisy, g)
        torch.cuda.synchronize()
        mse = lambda a: float(((a.double() - ref.double()) ** 2).mean())  # noqa: E731
        a, b = mse(noisy), mse(den)
        print(f"1920x1080 quality against {args.ref_spp} spp ({st.kernel_ms:.1f} ms): MSE noisy 16 spp {a:.6e}, denoised {b:.6e}, ratio {b / a:.4f}",
              flush=True)
        result["quality"] = {"ref_spp": args.ref_spp, "ref_ms": st.kernel_ms, "mse_noisy": a, "mse_denoised": b, "ratio": b / a}
        dn.close()
        ds.close()
    print(json.dumps(result), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
