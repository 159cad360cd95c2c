#!/usr/bin/env python3
"""The noise estimate of progressive rendering (rayz_hip_progressive_track_noise / _noise / _run_until) on an
MI355X: what tracking costs, against what, and what render-until-converged spends.  Config 3 (randomBouncing a,b in [-50,50):
10,003 spheres, 50 bounces, f32, BVH) at 1920x1080.

1. The fold.  accumulate_moments_kernel (a tracked handle) against accumulate_kernel (an untracked one), no preview written, for
   one-chunk passes (64 spp in chunks of 16: the first pass starts from +0 and only writes acc and Q, the later ones read and
   write them) and for one whole-schedule pass (256 spp, 16 chunks).  All timing is by HIP events: a pass is bracketed by events
   on the caller's stream, and the trace kernel of the SAME pass by the library's own events (rayz_hip_progressive_info); their
   difference is what follows the trace kernel in the pass — the fold kernel, with the work-queue counter's clear and the launch
   gaps, which both forms pay alike.  Median [min, max] over --reps handles.  Next to each: a device-to-device copy, in the same
   process and timed with events the same way, that moves the fold's COMPULSORY BYTES per pixel — 16 per chunk, plus acc (16) and
   Q (32) written, plus both read by a pass that is not the first — as a copy of half as many bytes (read + write), and the
   ratio fold / copy.
2. The evaluation.  noise_eval_kernel with both per-pixel outputs and no summary (nothing blocks): 48 B read and 8 B written per
   pixel, against the copy of those bytes.
3. What render-until-converged spends.  run_until at rel_error 0.05 and 0.02 (at most 1 % of the pixels unconverged, passes of 64
   samples, up to --max-spp): the samples per pixel it stops at, the fraction still unconverged, the time.

    python tools/noise_bench.py [--reps 7] [--copy-reps 100] [--max-spp 1024] [--width 1920] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rayz_amd import capi, render, tracer  # noqa: E402

ALL = 0xFFFFFFFF


def stat(ms):
    return {"ms": statistics.median(ms), "min": min(ms), "max": max(ms)}


def copy_ms(nbytes_moved, stream, reps, warmup=10):
    """A device copy that reads and writes `nbytes_moved` in all: median, min, max of event-bracketed copies."""
    half = max(nbytes_moved // 2, 1)
    src = torch.empty(half, dtype=torch.uint8, device="cuda")
    dst = torch.empty(half, dtype=torch.uint8, device="cuda")
    ms = []
    with torch.cuda.stream(stream):
        for i in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            dst.copy_(src)
            e1.record(stream)
            e1.synchronize()
            if i >= warmup:
                ms.append(e0.elapsed_time(e1))
    return stat(ms)


def passes(ds, cam, p, tracked, mins, stream):
    """Steps one handle to the end with min_samples `mins` (the last repeats), no preview.  Per pass: (chunks, events around the
    pass, the trace kernel's own events, their difference)."""
    pr = ds.progressive(cam, p, track_noise=tracked)
    rows, trace_so_far, i = [], 0.0, 0
    try:
        while not pr.done:
            c0 = pr.chunks_done
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            pr.step(mins[min(i, len(mins) - 1)], 0, stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            total = e0.elapsed_time(e1)
            trace = pr.stats().kernel_ms  # summed over the passes so far
            rows.append((pr.chunks_done - c0, total, trace - trace_so_far, total - (trace - trace_so_far)))
            trace_so_far = trace
            i += 1
    finally:
        pr.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--copy-reps", type=int, default=100)
    ap.add_argument("--max-spp", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    render.init(0)
    stream = torch.cuda.Stream()
    t = tracer.randomBouncing(args.width, -50, 50, seed=42)  # config 3
    t.samples_per_px, t.max_bounces = 64, 50
    t.set_gpu(render_seed=1, traversal=capi.TRAVERSAL_BVH)
    sd, cam, base = t.scene_desc(), t.camera_desc(), t.params()
    base.tmin, base.chunk_spp = 1e-3, 16
    n = base.width * base.height
    ds = render.DeviceScene(sd)
    result = {"width": base.width, "height": base.height, "reps": args.reps, "fold": {}, "run_until": []}

    def params(spp):
        p = capi.RenderParams.from_buffer_copy(bytes(base))
        p.samples_per_px = spp
        return p

    print(f"{base.width}x{base.height}, config 3 through the BVH, f32", flush=True)
    passes(ds, cam, params(64), True, [0], stream)  # warm-up: scene upload, workspace, the kernels' code objects
    # ---- 1. the fold ----
    cases = [("one chunk, first pass", 64, [0], lambda r: r[:1], 16 + 16, 16 + 48),
             ("one chunk, later pass", 64, [0], lambda r: r[1:], 16 + 32, 16 + 96),
             ("whole schedule (16 chunks)", 256, [ALL], lambda r: r, 16 * 16 + 16, 16 * 16 + 48)]
    for name, spp, mins, pick, b_plain, b_tracked in cases:
        row = {}
        for tracked, per_px in ((False, b_plain), (True, b_tracked)):
            fold, trace = [], []
            for _ in range(args.reps):
                for _, _, tr, rest in pick(passes(ds, cam, params(spp), tracked, mins, stream)):
                    fold.append(rest)
                    trace.append(tr)
            cp = copy_ms(n * per_px, stream, args.copy_reps)
            f = stat(fold)
            row["tracked" if tracked else "untracked"] = {"bytes_per_pixel": per_px, "fold": f, "copy": cp, "ratio_to_copy": f["ms"] / cp["ms"],
                                                          "trace_ms": statistics.median(trace)}
            print(f"  {name:27s} {'tracked  ' if tracked else 'untracked'}: after the trace kernel ({statistics.median(trace):8.3f} ms) "
                  f"{f['ms']:.4f} ms [{f['min']:.4f}, {f['max']:.4f}]; copy of its {per_px} B/pixel {cp['ms']:.4f} ms "
                  f"[{cp['min']:.4f}, {cp['max']:.4f}] ({n * per_px / cp['ms'] / 1e9:.2f} TB/s); ratio {f['ms'] / cp['ms']:.2f}", flush=True)
        row["tracked_over_untracked"] = row["tracked"]["fold"]["ms"] / row["untracked"]["fold"]["ms"]
        row["bytes_ratio"] = b_tracked / b_plain
        print(f"  {name:27s} tracked / untracked: {row['tracked_over_untracked']:.2f} in time, {row['bytes_ratio']:.2f} in bytes", flush=True)
        result["fold"][name] = row
    # ---- 2. the evaluation ----
    pr = ds.progressive(cam, params(64), track_noise=True)
    try:
        pr.step(ALL)
        pr.stats()
        ms = []
        for i in range(10 + args.copy_reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            pr.noise(var=True, rel2=True, summary=False, stream=stream.cuda_stream)
            e1.record(stream)
            e1.synchronize()
            if i >= 10:
                ms.append(e0.elapsed_time(e1))
        t0 = time.perf_counter()
        sm, _, _ = pr.noise()
        blocking = 1e3 * (time.perf_counter() - t0)
    finally:
        pr.close()
    ev, cp = stat(ms), copy_ms(n * 56, stream, args.copy_reps)
    result["eval"] = {"bytes_per_pixel": 56, "eval": ev, "copy": cp, "ratio_to_copy": ev["ms"] / cp["ms"], "with_summary_wall_ms": blocking}
    print(f"  evaluation (var and rel2 written, the summary's clear included): {ev['ms']:.4f} ms [{ev['min']:.4f}, {ev['max']:.4f}]; copy of its "
          f"56 B/pixel {cp['ms']:.4f} ms; ratio {ev['ms'] / cp['ms']:.2f}; with the summary, host wall time {blocking:.3f} ms", flush=True)
    # ---- 3. what run_until spends ----
    for rel in (0.05, 0.02):
        pr = ds.progressive(cam, params(args.max_spp), track_noise=True)
        try:
            t0 = time.perf_counter()
            sm = pr.render_until(rel_error=rel, max_unconverged_fraction=0.01, min_samples_per_pass=64)
            wall = 1e3 * (time.perf_counter() - t0)
            trace = pr.stats().kernel_ms
            row = {"rel_error": rel, "samples_done": sm.samples_done, "max_spp": args.max_spp, "schedule_ended": pr.done,
                   "unconverged_fraction": sm.unconverged / sm.pixels, "mean_var": sm.mean_var, "wall_ms": wall, "trace_ms": trace}
        finally:
            pr.close()
        print(f"  run_until rel_error {rel}: stopped at {row['samples_done']} of {args.max_spp} spp"
              f"{' (schedule ended)' if row['schedule_ended'] else ''}, {100 * row['unconverged_fraction']:.2f} % unconverged, "
              f"{wall:.1f} ms wall, {trace:.1f} ms of it tracing", flush=True)
        result["run_until"].append(row)
    ds.close()
    print(json.dumps(result), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
