#!/usr/bin/env python3
"""Adaptive passes (rayz_hip_progressive_set_adaptive / _run_adaptive) on an MI355X: what they save, what the
list costs, and how far stopping on a sample variance pulls the frozen pixels.  Config 3 (randomBouncing a,b in [-50,50): 10,003
spheres, 50 bounces, f32) at 1920x1080 x 1024 spp, through the BVH and through the flat list.

1. Saving.  run_adaptive against run_until(max_unconverged_fraction = 0) — unchanged by adaptive passes, so it is the baseline —
   at rel_error 0.05 and 0.02, both in passes of --pass-spp samples: samples traced and time.  Time is HIP events on the caller's
   stream around the whole run; one warm-up of each, then --reps runs in ALTERNATING order (A B A B ..); median [min, max].
2. Indirection cost.  One adaptive pass with every pixel active (the first pass: nothing can freeze before the second chunk) against
   the plain tracked pass over the same window, the same way: this prices the list indirection, the compact fold, the compaction
   and the blocking read of n_active.  The trace kernels' own times (the library's events) are reported beside them.
3. Bias.  At min_chunks 2, 4 and 8 (rel_error --bias-rel): over the frozen pixels and the channels with a positive variance
   estimate, the mean of z = (frozen value − 1024-spp value) / sqrt(var_ch), var_ch the pixel's own estimate at the chunk it froze
   at, with its standard error.  The 1024-spp frame contains the frozen pixel's own samples, so |z| is an underestimate of the
   error against the truth by the factor sqrt(1 − N_i / 1024) on average; the SIGN and the trend over min_chunks are the finding.

    python tools/adaptive_bench.py [--reps 3] [--width 1920] [--spp 1024] [--pass-spp 64] [--traversals bvh,flat] [--json FILE]"""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rayz_amd import capi, render, tracer  # noqa: E402


def stat(ms):
    return {"ms": statistics.median(ms), "min": min(ms), "max": max(ms), "n": len(ms)}


def timed(stream, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    r = fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--spp", type=int, default=1024)
    ap.add_argument("--pass-spp", type=int, default=64)
    ap.add_argument("--traversals", default="bvh,flat")
    ap.add_argument("--rel-errors", default="0.05,0.02")
    ap.add_argument("--bias-rel", type=float, default=0.05)
    ap.add_argument("--no-bias", action="store_true")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    render.init(0)
    stream = torch.cuda.Stream()
    t = tracer.randomBouncing(args.width, -50, 50, seed=42)  # config 3
    t.samples_per_px, t.max_bounces = args.spp, 50
    t.set_gpu(render_seed=1)
    sd, cam, base = t.scene_desc(), t.camera_desc(), t.params()
    base.tmin = 1e-3
    full = base.width * base.height * args.spp
    ds = render.DeviceScene(sd)
    result = {"width": base.width, "height": base.height, "spp": args.spp, "pass_spp": args.pass_spp, "reps": args.reps, "traversals": {}}
    s = stream.cuda_stream

    def params(trav):
        p = capi.RenderParams.from_buffer_copy(bytes(base))
        p.traversal = capi.TRAVERSAL_BVH if trav == "bvh" else capi.TRAVERSAL_LINEAR
        return p

    def run_adaptive(p, rel, min_chunks=None, out=None):
        pr = ds.progressive(cam, p, adaptive=True, min_chunks=min_chunks)
        try:
            ms, sm = timed(stream, lambda: pr.render_adaptive(rel_error=rel, min_samples_per_pass=args.pass_spp, out=out, stream=s))
            return {"ms": ms, "samples": sm.samples_traced, "passes": sm.passes, "active_left": sm.active, "trace_ms": pr.stats().kernel_ms}
        finally:
            pr.close()

    def run_until(p, rel):
        pr = ds.progressive(cam, p, track_noise=True)
        try:
            ms, sm = timed(stream, lambda: pr.render_until(rel_error=rel, max_unconverged_fraction=0.0, min_samples_per_pass=args.pass_spp,
                                                          stream=s))
            st = pr.stats()
            return {"ms": ms, "samples": st.primary_rays, "samples_done": sm.samples_done, "unconverged": sm.unconverged, "trace_ms": st.kernel_ms}
        finally:
            pr.close()

    def first_pass(p, adaptive):
        pr = ds.progressive(cam, p, adaptive=True) if adaptive else ds.progressive(cam, p, track_noise=True)
        try:
            if adaptive:
                ms, _ = timed(stream, lambda: pr.adaptive_step(min_samples=args.pass_spp, stream=s))
            else:
                ms, _ = timed(stream, lambda: pr.step(args.pass_spp, 0, s))
            return {"ms": ms, "trace_ms": pr.stats().kernel_ms}
        finally:
            pr.close()

    def alternate(a, b):  # one warm-up of each, then reps of A B A B ..
        a(), b()
        ra, rb = [], []
        for _ in range(args.reps):
            ra.append(a())
            rb.append(b())
        return ra, rb

    print(f"{base.width}x{base.height} x {args.spp} spp, config 3, f32, passes of {args.pass_spp} samples", flush=True)
    for trav in args.traversals.split(","):
        p = params(trav)
        row = {"saving": [], "indirection": None}
        for rel in (float(x) for x in args.rel_errors.split(",")):
            ad, un = alternate(lambda: run_adaptive(p, rel), lambda: run_until(p, rel))
            a, u = stat([r["ms"] for r in ad]), stat([r["ms"] for r in un])
            entry = {"rel_error": rel, "adaptive": {**ad[-1], "time": a}, "run_until": {**un[-1], "time": u}, "full_samples": full,
                     "samples_ratio": ad[-1]["samples"] / un[-1]["samples"], "time_ratio": a["ms"] / u["ms"]}
            row["saving"].append(entry)
            print(f"  {trav} rel_error {rel}: adaptive {ad[-1]['samples'] / full:6.1%} of {full} samples in {ad[-1]['passes']} passes, {a['ms']:.1f} ms "
                  f"[{a['min']:.1f}, {a['max']:.1f}], {ad[-1]['active_left']} pixels left active | run_until {un[-1]['samples'] / full:6.1%} "
                  f"(stopped at {un[-1]['samples_done']} spp, {un[-1]['unconverged']} unconverged), {u['ms']:.1f} ms [{u['min']:.1f}, {u['max']:.1f}] | "
                  f"samples x{entry['samples_ratio']:.3f}, time x{entry['time_ratio']:.3f}", flush=True)
        ad, pl = alternate(lambda: first_pass(p, True), lambda: first_pass(p, False))
        a, u = stat([r["ms"] for r in ad]), stat([r["ms"] for r in pl])
        ta, tu = stat([r["trace_ms"] for r in ad]), stat([r["trace_ms"] for r in pl])
        row["indirection"] = {"adaptive_pass": a, "plain_pass": u, "adaptive_trace": ta, "plain_trace": tu, "ratio": a["ms"] / u["ms"]}
        print(f"  {trav} one pass of {args.pass_spp} samples, every pixel active: adaptive {a['ms']:.2f} ms [{a['min']:.2f}, {a['max']:.2f}] "
              f"(trace kernel {ta['ms']:.2f}) | plain tracked {u['ms']:.2f} ms [{u['min']:.2f}, {u['max']:.2f}] (trace kernel {tu['ms']:.2f}) | "
              f"x{a['ms'] / u['ms']:.4f}", flush=True)
        result["traversals"][trav] = row
    if not args.no_bias:
        p = params(args.traversals.split(",")[0])
        ref = torch.empty((base.height, base.width, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ds.render_into(cam, p, ref.data_ptr())
        ds.sync()
        result["bias"] = []
        for mc in (2, 4, 8):
            pr = ds.progressive(cam, p, adaptive=True, min_chunks=mc)
            try:
                out = torch.empty_like(ref)
                sm = pr.render_adaptive(rel_error=args.bias_rel, min_samples_per_pass=args.pass_spp, out=out)
                var = pr.noise_rgb()
                pr.stats()
                frozen = pr.frozen_at() != 0
            finally:
                pr.close()
            ok = frozen[..., None] & (var > 0) & torch.isfinite(var)
            z = ((out - ref).double() / var.double().sqrt())[ok]
            n = int(z.numel())
            mean, sem = float(z.mean()), float(z.std()) / math.sqrt(max(n, 1))
            result["bias"].append({"min_chunks": mc, "rel_error": args.bias_rel, "frozen_pixels": int(frozen.sum()), "values": n,
                                   "mean_z": mean, "sem": sem, "samples_fraction": sm.samples_traced / full})
            print(f"  bias, min_chunks {mc} (rel_error {args.bias_rel}): mean z = {mean:+.4f} +- {sem:.4f} over {n} channel values of "
                  f"{int(frozen.sum())} frozen pixels; {sm.samples_traced / full:.1%} of the samples traced", flush=True)
    ds.close()
    print(json.dumps(result), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
