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
4. --guided: the variance-guided mode (rayz_hip_denoiser_run_guided) INSTEAD of 1-3.  Config 3 at 1920x1080, a
   16-spp frame from a tracked progressive handle stepped in 8 passes of one 2-sample chunk, its per-channel variance
   (rayz_hip_progressive_noise_rgb) and G-buffer; MSE against the --ref-spp frame of: the noisy frame, the unguided filter at its
   defaults, and the guided filter over sigma_color {1, 2, 4, 8} x var_floor {1e-6, 1e-4, 1e-2} x levels {3, 4, 5} — the sweep the
   guided defaults are taken from; then the per-level HIP-event times of both modes on that frame, same process, 5 levels.

5. --chain: chain guides and surface keys (rayz_hip_scene_query_camera_chain, rayz_hip_denoiser_set_keys) INSTEAD.
   Configs 2 and 3 at 1920x1080, the 16-spp tracked frame of --guided against --ref-spp; `run` and `run_guided` at their defaults
   with first-hit guides, with chain guides without keys and with chain guides plus keys, for max_fuzz 0, 0.25, 0.5 (max_depth 4):
   MSE over the whole frame and over the pixels whose FIRST hit is metal or glass.  Then the keys-off per-level HIP-event times of
   both modes (what the key compare costs a caller who does not use it is this build against its parent, run alternately).

6. --sampled: the sampled albedo (rayz_hip_scene_query_camera_sampled, QueryResult.with_albedo) INSTEAD.  Configs 2
   (whose camera has a defocus disk) and 3 at 1920x1080, the 16-spp tracked frame of --guided against --ref-spp, same seeds; `run`
   and `run_guided` at their defaults otherwise, with flags = DENOISE_ALBEDO on the first-hit G-buffer's point-sampled albedo, with
   flags = 0, and with flags = DENOISE_ALBEDO on the mean albedo over the frame's own 16 camera segments per pixel: MSE over the
   whole frame, and the two G-buffer queries' kernel times.

    python tools/denoise_bench.py [--reps 100] [--warmup 10] [--ref-spp 1024] [--paths] [--sizes 1920,3840] [--json FILE]
                                  [--guided | --chain | --sampled]"""
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


def level_times(dn, fn, levels, reps, warmup):
    """Median [min, max] of the handle's own event times over `reps` runs of fn(): [pack, level 0, ..]."""
    for _ in range(warmup):
        fn()
    rows = [[] for _ in range(levels + 1)]
    for _ in range(reps):
        fn()
        pk, ms = dn.timing()
        for k, x in enumerate([pk] + list(ms)):
            rows[k].append(x)
    return [(statistics.median(r), min(r), max(r)) for r in rows]


def guided(args):
    """Section 4 of the module docstring."""
    t = tracer.randomBouncing(1920, -50, 50, seed=42)  # config 3
    t.samples_per_px, t.max_bounces = 16, 50
    t.set_gpu(render_seed=1, traversal=capi.TRAVERSAL_BVH, chunk_spp=2)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    p.tmin = 1e-3
    w, h = p.width, p.height
    ds = render.DeviceScene(sd)
    pr = ds.progressive(cam, p, track_noise=True)
    noisy = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    passes = 0
    while not pr.done:
        pr.step(0, noisy.data_ptr())
        passes += 1
    var = pr.noise_rgb()
    st16 = pr.stats()
    sm, _, _ = pr.noise()
    g = ds.gbuffer(cam, p)
    ds.query_sync()
    print(f"{w}x{h} config 3: 16 spp in {passes} passes on a tracked handle ({st16.kernel_ms:.2f} ms of trace kernels); mean var {sm.mean_var:.4e}, "
          f"{sm.unconverged} of {sm.pixels} pixels unconverged at the default rel_error", flush=True)
    p.samples_per_px, p.chunk_spp = args.ref_spp, 0
    ref = torch.empty_like(noisy)
    torch.cuda.synchronize()
    ds.render_into(cam, p, ref.data_ptr())
    ref_ms = ds.sync().kernel_ms
    mse = lambda a: float(((a.double() - ref.double()) ** 2).mean())  # noqa: E731
    dn = render.Denoiser(w, h)
    out = torch.empty_like(noisy)
    res = {"size": f"{w}x{h}", "ref_spp": args.ref_spp, "ref_ms": ref_ms, "passes": passes, "mse_noisy": mse(noisy), "sweep": []}
    dn.run(noisy, g, out=out)
    torch.cuda.synchronize()
    res["mse_unguided_defaults"] = mse(out)
    print(f"MSE against {args.ref_spp} spp ({ref_ms:.1f} ms): noisy {res['mse_noisy']:.6e}; unguided at its defaults {res['mse_unguided_defaults']:.6e} "
          f"(ratio {res['mse_unguided_defaults'] / res['mse_noisy']:.4f})", flush=True)
    best = None
    for levels in (3, 4, 5):
        for sc in (1.0, 2.0, 4.0, 8.0):
            for vf in (1e-6, 1e-4, 1e-2):
                dn.run_guided(noisy, var, g, out=out, levels=levels, sigma_color=sc, var_floor=vf)
                torch.cuda.synchronize()
                m = mse(out)
                row = {"levels": levels, "sigma_color": sc, "var_floor": vf, "mse": m, "ratio_to_noisy": m / res["mse_noisy"],
                       "ratio_to_unguided": m / res["mse_unguided_defaults"]}
                res["sweep"].append(row)
                if best is None or m < best["mse"]:
                    best = row
                print(f"  guided levels {levels} sigma_color {sc:g} var_floor {vf:g}: MSE {m:.6e} = {row['ratio_to_noisy']:.4f} x noisy, "
                      f"{row['ratio_to_unguided']:.4f} x unguided", flush=True)
    res["best"] = best
    print(f"best: {best}", flush=True)
    d = capi.DENOISE_GUIDED_DEFAULTS
    dn.run_guided(noisy, var, g, out=out)
    torch.cuda.synchronize()
    res["mse_guided_defaults"] = mse(out)
    print(f"guided at the shipped defaults (levels {d['levels']}, sigma_color {d['sigma_color']:g}, var_floor {d['var_floor']:g}): "
          f"MSE {res['mse_guided_defaults']:.6e}", flush=True)
    L = 5
    a = level_times(dn, lambda: dn.run(noisy, g, out=out, levels=L), L, args.reps, args.warmup)
    b = level_times(dn, lambda: dn.run_guided(noisy, var, g, out=out, levels=L), L, args.reps, args.warmup)
    res["times"] = []
    for k in range(L + 1):
        what = "pack" if k == 0 else f"level {k - 1} (stride {1 << (k - 1)}{', last' if k == L else ''})"
        print(f"  {what:24s}: unguided {a[k][0]:.4f} ms [{a[k][1]:.4f}, {a[k][2]:.4f}]   guided {b[k][0]:.4f} ms [{b[k][1]:.4f}, {b[k][2]:.4f}]   "
              f"= {b[k][0] / a[k][0]:.2f} x", flush=True)
        res["times"].append({"what": what, "unguided_ms": a[k][0], "unguided_min": a[k][1], "unguided_max": a[k][2], "guided_ms": b[k][0],
                             "guided_min": b[k][1], "guided_max": b[k][2]})
    ta, tb = sum(x[0] for x in a), sum(x[0] for x in b)
    res["kernels_unguided_ms"], res["kernels_guided_ms"] = ta, tb
    print(f"  whole {L}-level pass, kernels: unguided {ta:.4f} ms, guided {tb:.4f} ms = {tb / ta:.2f} x", flush=True)
    pr.close()
    dn.close()
    ds.close()
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


def chain(args):
    """Section 5 of the module docstring."""
    res = {}
    for cfg, make in (("2", lambda: tracer.randomBouncing(1920, seed=42)), ("3", lambda: tracer.randomBouncing(1920, -50, 50, seed=42))):
        t = make()
        t.samples_per_px, t.max_bounces = 16, 50
        t.set_gpu(render_seed=1, traversal=capi.TRAVERSAL_BVH, chunk_spp=2)
        sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
        p.tmin = 1e-3
        w, h = p.width, p.height
        ds = render.DeviceScene(sd)
        pr = ds.progressive(cam, p, track_noise=True)
        noisy = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        while not pr.done:
            pr.step(0, noisy.data_ptr())
        var = pr.noise_rgb()
        pr.stats()
        first = ds.gbuffer(cam, p)
        ds.query_sync()
        kinds = torch.tensor([sd.materials[i].kind for i in range(sd.n_materials)], device="cuda")
        spec = (first.index >= 0) & (kinds[first.material.clamp(min=0).long()] != capi.MAT_DIFFUSE)
        p.samples_per_px, p.chunk_spp = args.ref_spp, 0
        ref = torch.empty_like(noisy)
        torch.cuda.synchronize()
        ds.render_into(cam, p, ref.data_ptr())
        ds.sync()
        err = lambda a: ((a.double() - ref.double()) ** 2).mean(dim=2)  # noqa: E731

        def both(a):  # (a run is asynchronous on the library's stream: wait before torch reads its output)
            if isinstance(a, tuple):
                a = a[0]
            torch.cuda.synchronize()
            return float(err(a).mean()), float(err(a)[spec].mean())

        dn = render.Denoiser(w, h)
        rows = {"noisy": both(noisy), "run first-hit": both(dn.run(noisy, first)), "run_guided first-hit": both(dn.run_guided(noisy, var, first))}
        for fuzz in (0.0, 0.25, 0.5):
            g = ds.gbuffer(cam, p, chain=dict(max_depth=4, max_fuzz=fuzz))
            ds.query_sync()
            for keys, kname in ((None, "no keys"), ("auto", "keys")):
                rows[f"run chain max_fuzz {fuzz} {kname}"] = both(dn.run(noisy, g, keys=keys))
                rows[f"run_guided chain max_fuzz {fuzz} {kname}"] = both(dn.run_guided(noisy, var, g, keys=keys))
        print(f"config {cfg}, {w}x{h}, 16 spp against {args.ref_spp} spp; {float(spec.float().mean()):.3f} of the pixels first hit metal or glass.  "
              "MSE whole frame | over those pixels (ratio to the noisy frame's)", flush=True)
        for k, (a, b) in rows.items():
            print(f"  {k:44s} {a:.6e} ({a / rows['noisy'][0]:.3f}) | {b:.6e} ({b / rows['noisy'][1]:.3f})", flush=True)
        res[cfg] = rows
        if cfg == "3":
            out = torch.empty_like(noisy)
            for name, fn in (("run", lambda: dn.run(noisy, first, out=out)), ("run_guided", lambda: dn.run_guided(noisy, var, first, out=out))):
                rows_t = level_times(dn, fn, 5, args.reps, args.warmup)
                print(f"  keys off, {name}: pack {rows_t[0][0]:.4f} ms, levels " + ", ".join(f"{m:.4f} [{lo:.4f}, {hi:.4f}]" for m, lo, hi in rows_t[1:]) +
                      f"; sum {sum(r[0] for r in rows_t):.4f} ms", flush=True)
                res[f"keys_off_{name}_ms"] = [r[0] for r in rows_t]
        dn.close(), pr.close(), ds.close()
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


def sampled(args):
    """Section 6 of the module docstring."""
    res = {}
    for cfg, make in (("2", lambda: tracer.randomBouncing(1920, seed=42)), ("3", lambda: tracer.randomBouncing(1920, -50, 50, seed=42))):
        t = make()
        t.samples_per_px, t.max_bounces = 16, 50
        t.set_gpu(render_seed=1, traversal=capi.TRAVERSAL_BVH, chunk_spp=2)
        sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
        p.tmin = 1e-3
        w, h = p.width, p.height
        ds = render.DeviceScene(sd)
        pr = ds.progressive(cam, p, track_noise=True)
        noisy = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        while not pr.done:
            pr.step(0, noisy.data_ptr())
        var = pr.noise_rgb()
        pr.stats()
        first = ds.gbuffer(cam, p)
        first_ms = ds.query_sync().kernel_ms
        smp = ds.gbuffer_sampled(cam, p, outputs=("albedo", "hits"))  # the frame's own camera segments: same seed, same 16 spp
        smp_ms = ds.query_sync().kernel_ms
        mixed = float(((smp.hits > 0) & (smp.hits < 16)).float().mean())
        moved = float(((smp.albedo - first.albedo).abs().amax(dim=2) > 1e-3).float().mean())
        guide = first.with_albedo(smp.albedo)
        q = capi.RenderParams.from_buffer_copy(p)
        q.samples_per_px, q.chunk_spp = args.ref_spp, 0
        ref = torch.empty_like(noisy)
        torch.cuda.synchronize()
        ds.render_into(cam, q, ref.data_ptr())
        ds.sync()

        def mse(a):  # (a run is asynchronous on the library's stream: wait before torch reads its output)
            if isinstance(a, tuple):
                a = a[0]
            torch.cuda.synchronize()
            return float(((a.double() - ref.double()) ** 2).mean())

        dn = render.Denoiser(w, h)
        A = capi.DENOISE_ALBEDO
        rows = {"noisy": mse(noisy)}
        for name, fn in (("run", lambda g, flags: dn.run(noisy, g, flags=flags)), ("run_guided", lambda g, flags: dn.run_guided(noisy, var, g, flags=flags))):
            rows[f"{name} point-sampled albedo"] = mse(fn(first, A))
            rows[f"{name} flags = 0"] = mse(fn(first, 0))
            rows[f"{name} sampled albedo"] = mse(fn(guide, A))
        print(f"config {cfg}, {w}x{h}, 16 spp against {args.ref_spp} spp, camera with{'' if cam.defocus else 'out'} a defocus disk; first-hit G-buffer "
              f"{first_ms:.3f} ms, sampled G-buffer (n = 16, albedo and hits) {smp_ms:.3f} ms; {100 * mixed:.2f} % of the pixels are hit by some samples "
              f"only, {100 * moved:.2f} % have a sampled albedo more than 1e-3 from the point sample.  MSE (ratio to the noisy frame's)", flush=True)
        for k, a in rows.items():
            print(f"  {k:36s} {a:.6e} ({a / rows['noisy']:.4f})", flush=True)
        res[cfg] = {"rows": rows, "first_ms": first_ms, "sampled_ms": smp_ms, "mixed_share": mixed, "moved_share": moved}
        dn.close(), pr.close(), ds.close()
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--levels", type=int, default=5)
    ap.add_argument("--paths", action="store_true")
    ap.add_argument("--sizes", default="1920,3840")
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    ap.add_argument("--guided", action="store_true", help="the variance-guided mode's sweep and level times instead")
    ap.add_argument("--chain", action="store_true", help="chain guides and surface keys against first-hit guides instead")
    ap.add_argument("--sampled", action="store_true", help="demodulation by the sampled albedo against the point sample and flags = 0 instead")
    args = ap.parse_args()
    render.init(0)
    if args.guided:
        return guided(args)
    if args.sampled:
        return sampled(args)
    if args.chain:
        return chain(args)
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
