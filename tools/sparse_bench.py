#!/usr/bin/env python3
"""Sparse renders (rayz_hip_scene_render_pixels) on an MI355X: what a lattice frame costs to trace, and what it is
worth under the upscaler, against the low-resolution frame of `lowres_camera` that it replaces.

Configs 2 and 3 at 1920x1080, 16 spp, f = 2 and 4.  All times are the library's own HIP events (RayzRenderStats.kernel_ms; a sparse
render's covers its range check — with the host's wait for the 4-byte count —, its trace and its resolve).

1. Trace time.  Through the BVH and through the flat list, alternating in one process --rounds times (median [min, max]):
     full      the whole frame (its time / f² is what a lattice of 1 / f² of the pixels would cost if tracing scaled with pixels);
     lowres    the `lowres_camera` frame of the lattice's size: every pixel the mean over an f x f block's footprint;
     rows      the lattice of phase (0, 0), listed row by row;
     tiles     the same lattice dealt in 8x8 tiles.
2. Error against --ref-spp samples per pixel (BVH; --seeds render seeds, median [min, max] of the MSE), of
     lowres + Upscaler.run          and          lattice + Upscaler.run(phase=...),
   each with and without DENOISE_ALBEDO in the upscaler, unfiltered and followed by Denoiser.run_guided on the variance the
   upscaler hands on; and the bilinear interpolation of the lowres frame, for scale.  Both frames are traced with the same
   schedule (16 spp in 8 chunks, for the variance).

    python tools/sparse_bench.py [--rounds 5] [--seeds 3] [--ref-spp 1024] [--json FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rayz_amd import capi, render, tracer  # noqa: E402

WIDTH, SPP = 1920, 16


def mmm(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def fmt(s, unit="ms"):
    return f"{s['median']:.3f} [{s['min']:.3f}, {s['max']:.3f}] {unit}" if unit else f"{s['median']:.4e} [{s['min']:.4e}, {s['max']:.4e}]"


def with_params(p, **kw):
    q = capi.RenderParams.from_buffer_copy(p)
    for k, v in kw.items():
        setattr(q, k, v)
    return q


def full_frame(ds, cam, p, out):
    ds.render_into(cam, p, out.data_ptr())
    return ds.sync().kernel_ms


def tracked(ds, cam, p):
    """A frame and its per-channel variance from a tracked progressive handle, as tools/upscale_bench.py takes them."""
    pr = ds.progressive(cam, p, track_noise=True)
    frame = torch.empty((p.height, p.width, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    pr.step(0xFFFFFFFF, frame.data_ptr())
    var = pr.noise_rgb()
    pr.stats()
    torch.cuda.synchronize()
    pr.close()
    return frame, var


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=3)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    args = ap.parse_args()
    render.init(0)
    result = {"rounds": args.rounds, "seeds": args.seeds, "ref_spp": args.ref_spp, "configs": {}}
    for cfg, make in (("2", lambda: tracer.randomBouncing(WIDTH, seed=42)), ("3", lambda: tracer.randomBouncing(WIDTH, -50, 50, seed=42))):
        t = make()
        t.samples_per_px, t.max_bounces = SPP, 50
        t.set_gpu(render_seed=1, traversal=capi.TRAVERSAL_BVH)
        sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
        p.tmin = 1e-3
        W, H = p.width, p.height
        ds = render.DeviceScene(sd)
        res = {"trace": {}, "error": {}}
        print(f"config {cfg}, {W}x{H}, {SPP} spp", flush=True)
        # ---- 1. trace time ---------------------------------------------------------------------------------------------------
        full = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        for trav, name in ((capi.TRAVERSAL_BVH, "bvh"), (capi.TRAVERSAL_LINEAR, "flat")):
            q = with_params(p, traversal=trav)
            variants = {"full": lambda: full_frame(ds, cam, q, full)}
            keep = []
            for f in (2, 4):
                cam_lo, q_lo = render.lowres_camera(cam, f), render.lowres_params(q, f)
                lo = torch.empty((q_lo.height, q_lo.width, 3), dtype=torch.float32, device="cuda")
                variants[f"f{f} lowres"] = lambda cam_lo=cam_lo, q_lo=q_lo, lo=lo: full_frame(ds, cam_lo, q_lo, lo)
                for order in ("rows", "tiles"):
                    pixels, dest = render.lattice_pixels(W, H, f, (0, 0), order=order, device="cuda")
                    keep.append((pixels, dest))

                    def lattice(pixels=pixels, dest=dest, lo=lo):
                        ds.render_pixels(cam, q, pixels, dest=dest, out=lo)
                        return ds.sync().kernel_ms

                    variants[f"f{f} {order}"] = lattice
            torch.cuda.synchronize()
            times = {k: [] for k in variants}
            for r in range(args.rounds + 1):  # (round 0 warms every variant up)
                for k, fn in variants.items():
                    ms = fn()
                    if r:
                        times[k].append(ms)
            rows = {k: mmm(v) for k, v in times.items()}
            res["trace"][name] = rows
            print(f"  trace time, {name}:", flush=True)
            for k, s in rows.items():
                f2 = int(k[1]) ** 2 if k != "full" else 1
                note = "" if k == "full" else f"   = {s['median'] / (rows['full']['median'] / f2):.2f} x full / f²"
                print(f"    {k:<10} {fmt(s)}{note}", flush=True)
        # ---- 2. error against the reference -------------------------------------------------------------------------------------
        ref = torch.empty((H, W, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ref_ms = full_frame(ds, cam, with_params(p, samples_per_px=args.ref_spp), ref)
        mse = lambda a: float(((a.double() - ref.double()) ** 2).mean())  # noqa: E731
        g_hi = ds.gbuffer(cam, p)
        ds.query_sync()
        dn = render.Denoiser(W, H)
        print(f"  error against {args.ref_spp} spp ({ref_ms:.1f} ms), MSE median [min, max] over {args.seeds} render seeds:", flush=True)
        for f in (2, 4):
            phase = render.phase_sequence(f)[0]
            cam_lo, p_lo = render.lowres_camera(cam, f), render.lowres_params(p, f)
            g_blk = ds.gbuffer(cam_lo, p_lo)
            ds.query_sync()
            g_lat = g_hi.lattice(f, phase)
            pixels, dest = render.lattice_pixels(W, H, f, phase, device="cuda")
            up = render.Upscaler(W, H, f)
            rows = {}
            for seed in range(1, args.seeds + 1):
                q = with_params(p, seed=seed, chunk_spp=SPP // 8)
                blk, blk_var = tracked(ds, cam_lo, render.lowres_params(q, f))
                lat = torch.empty_like(blk)
                lat_var = torch.empty_like(blk)
                torch.cuda.synchronize()
                ds.render_pixels(cam, q, pixels, dest=dest, out=lat, var=lat_var)
                ds.sync()
                bil = torch.nn.functional.interpolate(blk.permute(2, 0, 1)[None], size=(H, W), mode="bilinear", align_corners=False)[0]
                rows.setdefault("lowres, bilinear interpolation", []).append(mse(bil.permute(1, 2, 0)))
                for src, rgb, var, g_lo, ph in (("lowres ", blk, blk_var, g_blk, None), ("lattice", lat, lat_var, g_lat, phase)):
                    for flags, tag in ((capi.DENOISE_ALBEDO, "DENOISE_ALBEDO"), (0, "flags = 0      ")):
                        out, var_out, stage = up.run(rgb, g_lo, g_hi, var_rgb=var, stage=True, phase=ph, flags=flags)
                        torch.cuda.synchronize()
                        rows.setdefault(f"{src} + upscale, {tag}", []).append(mse(out))
                        den = dn.run_guided(out, var_out, g_hi)
                        torch.cuda.synchronize()
                        rows.setdefault(f"{src} + upscale, {tag} + run_guided", []).append(mse(den))
                        rows.setdefault(f"{src} stage 1+2 share", []).append(float((stage > 0).float().mean()))
            stats = {k: mmm(v) for k, v in rows.items()}
            res["error"][str(f)] = stats
            print(f"    f = {f} (phase {phase}):", flush=True)
            for k, s in stats.items():
                print(f"      {k:<52} {fmt(s, '')}", flush=True)
            up.close()
        dn.close()
        ds.close()
        result["configs"][cfg] = res
    print(json.dumps(result), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(result, fh, indent=1)


if __name__ == "__main__":
    main()
