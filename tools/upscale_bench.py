#!/usr/bin/env python3
"""Guided upscaling (rayz_hip_upscaler_*) on an MI355X: what it costs, against what, and what it buys.

1. Cost.  1920x1080, configs 2 and 3, f = 2 and f = 4: the low-resolution 16-spp frame, its per-channel variance and the two real
   G-buffers.  Both parts of a run are bracketed by the handle's own HIP events (rayz_hip_upscaler_timing): the pack launches and
   the reconstruction launch, median [min, max] of --reps runs after --warmup, colour only and with variance + stage map.  Next
   to each: a device-to-device copy, in the same process and timed with events, that moves the launch's COMPULSORY bytes (DESIGN.md
   §6 derives them) — per full pixel 52 + 48/f² (colour only) or 65 + 64/f² (variance and stage map too) for the reconstruction,
   per low-resolution pixel 116 (or 160) for the pack —, and the ratio.  This build has the direct form only, so there is no
   direct-against-staged comparison to make.
2. What it buys.  Against the --ref-spp frame, the MSE and the total device time (trace kernels + G-buffer queries + filter kernels,
   each by the library's own events) of
     (a) the full-resolution 16-spp frame + run_guided;
     (b) low-resolution trace -> low-resolution run_guided -> upscale;
     (c) low-resolution trace -> upscale with variance -> full-resolution run_guided;
     (d) low-resolution trace -> bilinear torch.nn.functional.interpolate, the naive baseline;
   with the same seeds, at two sample budgets: equal spp (16 at low resolution) and equal traced samples (f²·16 at low resolution).
   Every frame comes from a tracked progressive handle stepped in 8 passes (its variance is rayz_hip_progressive_noise_rgb).  The
   share of the pixels in stages 1 and 2 is reported with (c).  (b) and (c) run the upscaler with RAYZ_DENOISE_ALBEDO, (b0) and (c0)
   with flags = 0: no demodulation in the upscaler (the denoiser keeps its defaults).  The cost rows are measured with the flag: the
   costlier state, which reads both albedos.

3. With --footprint: the footprint albedo (rayz_hip_upscaler_footprint_albedo).  In the same run and with the same
   seeds, beside the rows above: (cF) and (bF), which are (c) and (b) with the filtered albedo handed to the upscaler in place of the
   low-resolution G-buffer's — for (bF) also to the low-resolution run_guided, which demodulates by the same point sample; their
   device time includes the footprint launch.  And the launch itself, bracketed by the handle's own events
   (rayz_hip_upscaler_footprint_timing), against a device copy of its compulsory bytes — per full pixel 16 (index and albedo) +
   (28 + the count's byte) / f² (the low-resolution index and albedo in, the albedo out) —, median [min, max] of --reps after --warmup.

4. With --sampled: the sampled albedo (rayz_hip_scene_query_camera_sampled, QueryResult.with_albedo).  In the same
   run and with the same seeds, beside the rows above, (b) and (c) demodulated (flags = RAYZ_DENOISE_ALBEDO) with a G-buffer's
   albedo replaced by the mean over camera segments: (bH), (cH) the FULL-SIZE G-buffer's, over the 16 segments per pixel a
   full-size 16-spp frame of the same seed would trace; (bL), (cL) the LOW-RESOLUTION G-buffer's, sampled through lowres_camera —
   whose pixel IS the f x f block — over the low-resolution frame's own segments (all of its spp); (bS), (cS) both.  MSE only; the
   sampled queries' kernel times are printed beside the first-hit G-buffers'.

    python tools/upscale_bench.py [--footprint] [--sampled] [--reps 100] [--warmup 10] [--ref-spp 1024] [--json FILE]"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rayz_amd import capi, render, tracer  # noqa: E402

WIDTH, SPP = 1920, 16


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


def handle_ms(handle, fn, reps, warmup):
    """Median [min, max] per entry of handle.timing() (flattened) over `reps` runs of fn()."""
    def flat():
        a, b = handle.timing()
        return [a] + (list(b) if isinstance(b, (list, tuple)) else [b])

    for _ in range(warmup):
        fn()
    rows = None
    for _ in range(reps):
        fn()
        t = flat()
        rows = rows or [[] for _ in t]
        for r, x in zip(rows, t):
            r.append(x)
    return [(statistics.median(r), min(r), max(r)) for r in rows]


def trace(ds, cam, p, spp):
    """A tracked `spp` frame in 8 passes: (frame, per-channel variance, ms of trace kernels)."""
    q = capi.RenderParams.from_buffer_copy(p)
    q.samples_per_px, q.chunk_spp = spp, max(spp // 8, 1)
    pr = ds.progressive(cam, q, track_noise=True)
    frame = torch.empty((q.height, q.width, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    while not pr.done:
        pr.step(0, frame.data_ptr())
    var = pr.noise_rgb()
    ms = pr.stats().kernel_ms
    torch.cuda.synchronize()
    pr.close()
    return frame, var, ms


def gbuffer(ds, cam, p):
    g = ds.gbuffer(cam, p)
    return g, ds.query_sync().kernel_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    ap.add_argument("--sampled", action="store_true", help="add the rows (bH), (cH), (bL), (cL), (bS), (cS) (DESIGN.md 4.25)")
    ap.add_argument("--footprint", action="store_true", help="add the rows (cF), (bF) and the footprint launch's cost (DESIGN.md 4.24)")
    args = ap.parse_args()
    render.init(0)
    stream = torch.cuda.Stream()
    result = {"reps": args.reps, "ref_spp": args.ref_spp, "configs": {}}
    for cfg, make in (("2", lambda: tracer.randomBouncing(WIDTH, seed=42)), ("3", lambda: tracer.randomBouncing(WIDTH, -50, 50, seed=42))):
        t = make()
        t.samples_per_px, t.max_bounces = SPP, 50
        t.set_gpu(render_seed=1, traversal=capi.TRAVERSAL_BVH)
        sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
        p.tmin = 1e-3
        W, H = p.width, p.height
        ds = render.DeviceScene(sd)
        q = capi.RenderParams.from_buffer_copy(p)
        q.samples_per_px = args.ref_spp
        ref = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ds.render_into(cam, q, ref.data_ptr())
        ref_ms = ds.sync().kernel_ms
        mse = lambda a: float(((a.double() - ref.double()) ** 2).mean())  # noqa: E731
        g_hi, g_hi_ms = gbuffer(ds, cam, p)
        dn = render.Denoiser(W, H)
        full, full_var, full_ms = trace(ds, cam, p, SPP)
        out_a = dn.run_guided(full, full_var, g_hi)
        dn_ms = sum(r[0] for r in handle_ms(dn, lambda: dn.run_guided(full, full_var, g_hi, out=out_a), 9, 2))
        a = {"mse": mse(out_a), "trace_ms": full_ms, "gbuffer_ms": g_hi_ms, "filter_ms": dn_ms, "total_ms": full_ms + g_hi_ms + dn_ms}
        print(f"config {cfg}, {W}x{H}, reference {args.ref_spp} spp ({ref_ms:.1f} ms).  MSE of the noisy {SPP}-spp frame {mse(full):.6e}", flush=True)
        print(f"  (a) full-resolution {SPP} spp + run_guided: MSE {a['mse']:.6e}; trace {full_ms:.3f} + G-buffer {g_hi_ms:.3f} + filter {dn_ms:.3f} "
              f"= {a['total_ms']:.3f} ms", flush=True)
        res = {"ref_ms": ref_ms, "mse_noisy": mse(full), "a": a, "factors": {}}
        g_hi_s = None
        if args.sampled:  # the full-size albedo over the camera segments of the full-size 16-spp frame (p: its seed and spp)
            s_hi = ds.gbuffer_sampled(cam, p, outputs=("albedo",))
            res["sampled_hi_ms"] = ds.query_sync().kernel_ms
            g_hi_s = g_hi.with_albedo(s_hi.albedo)
            print(f"  sampled full-size G-buffer (n = {SPP}, albedo): {res['sampled_hi_ms']:.3f} ms beside the first-hit G-buffer's {g_hi_ms:.3f} ms", flush=True)
        for f in (2, 4):
            cam_lo, p_lo = render.lowres_camera(cam, f), render.lowres_params(p, f)
            w, h = p_lo.width, p_lo.height
            g_lo, g_lo_ms = gbuffer(ds, cam_lo, p_lo)
            up = render.Upscaler(W, H, f)
            dn_lo = render.Denoiser(w, h)
            fr = {"budgets": {}}
            g_lo_f = fp_ms = None
            if args.footprint:  # the filtered albedo: of the G-buffers alone, the same for both budgets
                g_lo_f = copy.copy(g_lo)
                g_lo_f.albedo = up.footprint_albedo(g_lo, g_hi)
                fp_ms = up.footprint_timing()
            for budget, spp in (("equal spp", SPP), ("equal traced samples", SPP * f * f)):
                lo, lo_var, lo_ms = trace(ds, cam_lo, p_lo, spp)
                # (b), (c) with the upscaler's demodulation on (its default) and, as (b0), (c0), off
                rows = {}
                for tag, flags in (("", capi.DENOISE_ALBEDO), ("0", 0)):
                    # (b) filter at low resolution, then upscale
                    den_lo = dn_lo.run_guided(lo, lo_var, g_lo)
                    out_b = up.run(den_lo, g_lo, g_hi, flags=flags)
                    torch.cuda.synchronize()
                    b_dn = sum(r[0] for r in handle_ms(dn_lo, lambda: dn_lo.run_guided(lo, lo_var, g_lo, out=den_lo), 9, 2))
                    b_up = sum(r[0] for r in handle_ms(up, lambda: up.run(den_lo, g_lo, g_hi, out=out_b, flags=flags), 9, 2))
                    rows["b" + tag] = {"mse": mse(out_b), "filter_ms": b_dn + b_up, "total_ms": lo_ms + g_lo_ms + g_hi_ms + b_dn + b_up}
                    # (c) upscale with its variance, then filter at full resolution
                    up_c, var_c, stage = up.run(lo, g_lo, g_hi, var_rgb=lo_var, stage=True, flags=flags)
                    out_c = dn.run_guided(up_c, var_c, g_hi)
                    torch.cuda.synchronize()
                    c_up = sum(r[0] for r in handle_ms(up, lambda: up.run(lo, g_lo, g_hi, var_rgb=lo_var, out=up_c, var_out=var_c, stage=stage, flags=flags), 9, 2))
                    c_dn = sum(r[0] for r in handle_ms(dn, lambda: dn.run_guided(up_c, var_c, g_hi, out=out_c), 9, 2))
                    s1, s2 = float((stage == 1).float().mean()), float((stage == 2).float().mean())
                    rows["c" + tag] = {"mse": mse(out_c), "mse_upscaled_unfiltered": mse(up_c), "filter_ms": c_up + c_dn,
                                       "total_ms": lo_ms + g_lo_ms + g_hi_ms + c_up + c_dn, "stage1_share": s1, "stage2_share": s2}
                if args.footprint:  # (bF), (cF): (b), (c) on the filtered albedo; the footprint launch counts as a filter
                    den_lo = dn_lo.run_guided(lo, lo_var, g_lo_f)
                    out_b = up.run(den_lo, g_lo_f, g_hi, flags=capi.DENOISE_ALBEDO)
                    torch.cuda.synchronize()
                    b_dn = sum(r[0] for r in handle_ms(dn_lo, lambda: dn_lo.run_guided(lo, lo_var, g_lo_f, out=den_lo), 9, 2))
                    b_up = sum(r[0] for r in handle_ms(up, lambda: up.run(den_lo, g_lo_f, g_hi, out=out_b, flags=capi.DENOISE_ALBEDO), 9, 2))
                    rows["bF"] = {"mse": mse(out_b), "filter_ms": fp_ms + b_dn + b_up, "total_ms": lo_ms + g_lo_ms + g_hi_ms + fp_ms + b_dn + b_up}
                    up_c, var_c, stage = up.run(lo, g_lo_f, g_hi, var_rgb=lo_var, stage=True, flags=capi.DENOISE_ALBEDO)
                    out_c = dn.run_guided(up_c, var_c, g_hi)
                    torch.cuda.synchronize()
                    c_up = sum(r[0] for r in handle_ms(up, lambda: up.run(lo, g_lo_f, g_hi, var_rgb=lo_var, out=up_c, var_out=var_c, stage=stage,
                                                                         flags=capi.DENOISE_ALBEDO), 9, 2))
                    c_dn = sum(r[0] for r in handle_ms(dn, lambda: dn.run_guided(up_c, var_c, g_hi, out=out_c), 9, 2))
                    s1, s2 = float((stage == 1).float().mean()), float((stage == 2).float().mean())
                    rows["cF"] = {"mse": mse(out_c), "mse_upscaled_unfiltered": mse(up_c), "filter_ms": fp_ms + c_up + c_dn,
                                  "total_ms": lo_ms + g_lo_ms + g_hi_ms + fp_ms + c_up + c_dn, "stage1_share": s1, "stage2_share": s2}
                if args.sampled:  # (b), (c) on sampled albedos: H the full-size one, L the low-resolution one, S both
                    q_lo = capi.RenderParams.from_buffer_copy(p_lo)
                    q_lo.samples_per_px = spp  # (the low-resolution frame's own paths: trace() renders these params)
                    s_lo = ds.gbuffer_sampled(cam_lo, q_lo, outputs=("albedo",))
                    s_lo_ms = ds.query_sync().kernel_ms
                    g_lo_s = g_lo.with_albedo(s_lo.albedo)
                    for tag, gl, gh in (("H", g_lo, g_hi_s), ("L", g_lo_s, g_hi), ("S", g_lo_s, g_hi_s)):
                        den_lo = dn_lo.run_guided(lo, lo_var, gl)
                        out_b = up.run(den_lo, gl, gh, flags=capi.DENOISE_ALBEDO)
                        torch.cuda.synchronize()
                        rows["b" + tag] = {"mse": mse(out_b)}
                        up_c, var_c, stage = up.run(lo, gl, gh, var_rgb=lo_var, stage=True, flags=capi.DENOISE_ALBEDO)
                        out_c = dn.run_guided(up_c, var_c, gh)
                        torch.cuda.synchronize()
                        rows["c" + tag] = {"mse": mse(out_c), "mse_upscaled_unfiltered": mse(up_c)}
                    rows["sampled_lo_ms"] = s_lo_ms
                # (d) bilinear
                bil = lambda: torch.nn.functional.interpolate(lo.permute(2, 0, 1)[None], size=(H, W), mode="bilinear", align_corners=False)  # noqa: E731
                out_d = bil()[0].permute(1, 2, 0).contiguous()
                d_ms = event_ms(bil, stream, 9, 2)[0]
                d = {"mse": mse(out_d), "filter_ms": d_ms, "total_ms": lo_ms + d_ms}
                print(f"  f = {f}, {budget} ({spp} spp at {w}x{h}; trace {lo_ms:.3f} ms, G-buffers {g_lo_ms:.3f} + {g_hi_ms:.3f} ms):", flush=True)
                for tag, note in (("", "demodulated"), ("0", "flags = 0   ")) + ((("F", "footprint  "),) if args.footprint else ()):
                    b, c = rows["b" + tag], rows["c" + tag]
                    print(f"    (b{tag}) {note} run_guided low -> upscale:        MSE {b['mse']:.6e}  filters {b['filter_ms']:.3f} ms  total "
                          f"{b['total_ms']:.3f} ms = {b['total_ms'] / a['total_ms']:.3f} x (a)", flush=True)
                    print(f"    (c{tag}) {note} upscale + variance -> run_guided: MSE {c['mse']:.6e}  filters {c['filter_ms']:.3f} ms  total "
                          f"{c['total_ms']:.3f} ms = {c['total_ms'] / a['total_ms']:.3f} x (a); upscaled, unfiltered: MSE "
                          f"{c['mse_upscaled_unfiltered']:.6e}; stage 1: {100 * c['stage1_share']:.4f} %, stage 2: {100 * c['stage2_share']:.4f} % of the pixels",
                          flush=True)
                if args.sampled:
                    for tag, note in (("H", "full-size albedo sampled"), ("L", "low-resolution albedo sampled"), ("S", "both sampled")):
                        b, c = rows["b" + tag], rows["c" + tag]
                        print(f"    (b{tag}) {note}: MSE {b['mse']:.6e}    (c{tag}): MSE {c['mse']:.6e}; upscaled, unfiltered: MSE {c['mse_upscaled_unfiltered']:.6e}",
                              flush=True)
                    print(f"    sampled low-resolution G-buffer (n = {spp}, albedo): {rows['sampled_lo_ms']:.3f} ms", flush=True)
                print(f"    (d) bilinear interpolate:             MSE {d['mse']:.6e}  filter {d_ms:.3f} ms  total {d['total_ms']:.3f} ms", flush=True)
                fr["budgets"][budget] = {"spp": spp, "trace_ms": lo_ms, "gbuffer_lo_ms": g_lo_ms, **rows, "d": d}
                if spp != SPP:
                    continue
                # cost of the two launches against copies of their compulsory bytes
                n_hi, n_lo = W * H, w * h
                out2, var2 = torch.empty_like(up_c), torch.empty_like(var_c)
                fr["cost"] = {}
                for name, fn, rec_b, pack_b in (
                        ("colour only", lambda: up.run(lo, g_lo, g_hi, out=out2, flags=capi.DENOISE_ALBEDO), 52 + 48 / (f * f), 116),
                        ("colour + variance + stage map", lambda: up.run(lo, g_lo, g_hi, var_rgb=lo_var, out=out2, var_out=var2, stage=stage, flags=capi.DENOISE_ALBEDO), 65 + 64 / (f * f), 160)):
                    pack, rec = handle_ms(up, fn, args.reps, args.warmup)
                    row = {}
                    for what, tm, nbytes in (("pack", pack, int(n_lo * pack_b)), ("reconstruction", rec, int(n_hi * rec_b))):
                        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
                        dst = torch.empty_like(src)
                        cp = event_ms(lambda: dst.copy_(src), stream, args.reps, args.warmup)
                        print(f"    [{name}] {what}: {tm[0]:.4f} ms [{tm[1]:.4f}, {tm[2]:.4f}]; copy of its {nbytes / 1e6:.1f} MB: {cp[0]:.4f} ms "
                              f"[{cp[1]:.4f}, {cp[2]:.4f}] ({nbytes / cp[0] / 1e9:.2f} TB/s) = {tm[0] / cp[0]:.2f} x the copy", flush=True)
                        row[what] = {"ms": tm[0], "min": tm[1], "max": tm[2], "bytes": nbytes, "copy_ms": cp[0], "copy_min": cp[1], "copy_max": cp[2],
                                     "ratio_to_copy": tm[0] / cp[0]}
                    fr["cost"][name] = row
                if args.footprint:  # the footprint launch against a copy of its compulsory bytes
                    fp_out = torch.empty_like(g_lo.albedo)
                    fp_cnt = torch.empty((h, w), dtype=torch.uint8, device="cuda")
                    fr["footprint_cost"] = {}
                    for name, cnt in (("albedo only", False), ("albedo + count", fp_cnt)):
                        for _ in range(args.warmup):
                            up.footprint_albedo(g_lo, g_hi, out=fp_out, count=cnt)
                        ms = []
                        for _ in range(args.reps):
                            up.footprint_albedo(g_lo, g_hi, out=fp_out, count=cnt)
                            ms.append(up.footprint_timing())
                        tm = (statistics.median(ms), min(ms), max(ms))
                        nbytes = int(n_hi * (16 + (28 + (1 if cnt is not False else 0)) / (f * f)))
                        src = torch.empty(nbytes // 2, dtype=torch.uint8, device="cuda")
                        dst = torch.empty_like(src)
                        cp = event_ms(lambda: dst.copy_(src), stream, args.reps, args.warmup)
                        print(f"    [footprint, {name}] launch: {tm[0]:.4f} ms [{tm[1]:.4f}, {tm[2]:.4f}]; copy of its {nbytes / 1e6:.1f} MB: {cp[0]:.4f} ms "
                              f"[{cp[1]:.4f}, {cp[2]:.4f}] ({nbytes / cp[0] / 1e9:.2f} TB/s) = {tm[0] / cp[0]:.2f} x the copy", flush=True)
                        fr["footprint_cost"][name] = {"ms": tm[0], "min": tm[1], "max": tm[2], "bytes": nbytes, "copy_ms": cp[0], "copy_min": cp[1],
                                                      "copy_max": cp[2], "ratio_to_copy": tm[0] / cp[0]}
            res["factors"][str(f)] = fr
            up.close()
            dn_lo.close()
        dn.close()
        ds.close()
        result["configs"][cfg] = res
    print(json.dumps(result), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
