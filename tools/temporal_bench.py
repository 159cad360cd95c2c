#!/usr/bin/env python3
"""Temporal accumulation (rayz_hip_temporal_*) on an MI355X: what a step costs, against what, and what it buys.

Config 3 at 1920x1080 under a camera that pans --pan pixels per frame (px_origin moved along px_du) over --frames frames of 16 spp,
each from a tracked progressive handle with its own seed, in chunks of 2 samples (8 chunks: a variance estimate every frame), with
its camera G-buffer and its per-channel variance; and a --ref-spp frame of every camera.  Everything is made from seeds; nothing
is read from outside the tree.

(a) Cost.  The step kernel by the handle's own HIP events (rayz_hip_temporal_timing), median [min, max] of --reps steps after
    --warmup: a first frame (no history), a static step, a panned step; next to a device-to-device copy, timed with events in the
    same process, that moves the step's COMPULSORY BYTES — the current colour, variance and guides in (52 B per pixel), one history
    record in (64 B), the history, colour and variance out (88 B): 204 B per pixel, i.e. a copy of 102 B per pixel (read + write) —
    and the ratio step / copy.
(b) Quality.  Per frame, MSE against the --ref-spp frame of the same camera of: the raw frame, `run_guided` alone, the temporal
    step alone, and the temporal step followed by `run_guided` — at the shipped defaults.
(c) Coverage.  Per frame, the share of hit pixels that found history (length > spp).
(d) The sweep the defaults are to be chosen from: alpha_min x max_rel_dist, the mean over the panned frames of (b)'s temporal and
    temporal + guided MSE ratios to the raw frame, and of (c).

    python tools/temporal_bench.py [--frames 16] [--pan 3] [--spp 16] [--ref-spp 1024] [--reps 100] [--warmup 10] [--width 1920] [--json FILE]

--moments measures the moments mode instead (rayz_hip_temporal_step_moments), on the same sequence with every
frame rendered TWICE from one seed: in ONE chunk by `render_into` (no variance: what the moments step takes) and in two chunks by
a tracked progressive handle (frame + variance: what the plain step takes).
(a) Cost, plain and moments step by the handles' own HIP events in the same process, each beside a device copy of its compulsory
    bytes.  The moments step's: the current colour and guides in (40 B per pixel), one history record in — colour + length, normal
    + index, point, moments; the variance record is not read — (64 B), five history records, colour and variance out (104 B):
    208 B per pixel, a copy of 104 B per pixel.  Four states: a first frame (every workgroup stages its tile for the spatial
    estimate), a second static frame (W2 = 1/2 > w2_max: still every workgroup), a static and a panned step on a SETTLED history
    of --settle frames (W2 < w2_max: no workgroup, or only those at disocclusions).
(b) Quality.  Per frame, MSE against the --ref-spp frame of: the raw one-chunk frame; plain step on the two-chunk tracked frame,
    then `run_guided`; moments step on the one-chunk frame, then `run_guided`; and the share of hit pixels with W2 > w2_max.
(c) The sweep the defaults are to be chosen from: w2_max x min_taps, the first frame's and the mean over the later frames of (b)'s
    moments + guided MSE ratio to the raw frame.

    python tools/temporal_bench.py --moments [--settle 6] [the switches above]

--feedback measures the feedback of the filtered colour (rayz_hip_temporal_track_feedback / _feedback and
rayz_hip_denoiser_run_guided_tap) on --moments' one-chunk frames.
(a) Cost.  The feedback step beside the moments step, by the handles' own HIP events in the same process, in --moments' four
    states, each beside a device copy of its compulsory bytes: the feedback step reads one more history record, m1 (224 B per pixel
    against 208; what it writes to the v record changes its meaning, not its size).  The write kernel, by events around
    `Temporal.feedback`, beside a copy of its 44 B per pixel (12 B of the image and one 16-byte record in, the record out).  The
    guided run with a tap at level 1 beside the untapped run, both by the denoiser's own events (pack pass + levels).
(b) Quality.  Per frame, MSE against the --ref-spp frame of: the raw one-chunk frame; moments step + `run_guided`; and moments
    step on a feedback handle + `run_guided(tap_level=1)` with the tap fed back — both at the shipped defaults.

    python tools/temporal_bench.py --feedback [--settle 6] [the switches above]

--counts measures the counts step (rayz_hip_temporal_step_counts / _step_moments_counts).
(a) Cost.  The counts step beside the scalar step of the same mode, plain and moments, by the handles' own HIP events in the same
    process: a first frame, a static step, a panned step, on frames whose counts are an f = 2 lattice's (one pixel in four has 16,
    the others 0), each beside a device copy of its compulsory bytes — the twin's plus the 4 B per pixel of the count.
(b) Quality.  Per frame, MSE against the --ref-spp frame of three pipelines of (nearly) equal traced samples: an f = 2 lattice of
    16 spp cycling `phase_sequence`, rebuilt around its pixels by `Upscaler.run(phase=)` (what a pixel without samples and without
    history passes through), into a moments counts step, into `run_guided`; a `lowres_camera` frame of 16 spp in two tracked
    chunks, `Upscaler.run` with its variance, `run_guided`; and a full-resolution frame of 4 spp in one chunk through the moments
    step and `run_guided`.

    python tools/temporal_bench.py --counts [the switches above]

--cubic measures the cubic resampling mode (rayz_hip_temporal_set_resampling) beside the bilinear one, the two
alternating in one process on the same frames.
(a) Cost.  The panned step (frame 1 on frame 0's history) of a plain and of a moments handle in both modes, by the handles' own
    HIP events, each beside a device copy of the step's compulsory bytes (204 / 208 B per pixel; + 1 with the taken bytes, which the
    cubic handles here write), and the share of pixels that took the sixteen taps.  With --lib a second build's bilinear step
    cannot be loaded into the same process; run the tool once per build and compare the "bilinear" rows.
(b) Quality.  Per frame, MSE against the --ref-spp frame of the temporal step alone and of the step + `run_guided`, bilinear
    against cubic, on one-chunk frames through moments handles — over the whole frame, over the pixels whose first hit is diffuse
    and over those whose first hit is metal or glass (as tools/denoise_bench.py --chain splits them).  --pan 3 is the integer pan
    (fx = 0 up to rounding), --pan 2.5 a fractional one; --motion orbit turns look_from about the focus point by --pan pixel widths
    per frame, so that look_from and the view direction both change and the image motion depends on depth.  --config 2 | 3.

    python tools/temporal_bench.py --cubic [--config 3] [--motion pan|orbit] [--pan 2.5] [--lib PATH --lib-label NAME] [the switches above]

--background measures the background mode (rayz_hip_temporal_set_background) beside the input mode, the two
alternating in one process on the same frames; the input mode runs the kernels it always ran and is the yardstick.
(a) Cost.  The plain and the moments step in both modes — a first frame, a static step, a moved step — by the handles' own HIP
    events, each beside a device copy of the step's compulsory bytes (204 / 208 B per pixel), and the ratio accumulate / input.
(b) Quality.  Per frame, MSE against the --ref-spp frame of the temporal step alone and of the step + `run_guided`, input against
    accumulate, on one-chunk frames through moments handles — over the whole frame, and split into the background pixels' and
    the hit pixels' parts of it — and the share of background pixels that found history with their mean history length.
    --motion, --pan and --config as for --cubic.

    python tools/temporal_bench.py --background [--config 3] [--motion pan|orbit] [--pan 2.5] [--cost-only] [the switches above]

--clip measures the clip mode (rayz_hip_temporal_set_clip) beside the OFF mode, the two alternating in one
process on the same frames; the OFF mode runs the kernels it always ran and is the yardstick.
(a) Cost.  The MOVED step (the only one the mode changes) of a plain and of a moments handle, with the background passed through
    and accumulated, OFF against VARIANCE at the defaults with the clipped bytes written, by the handles' own HIP events, each
    beside a device copy of the step's compulsory bytes (204 / 208 B per pixel; + 1 with the map), the ratio variance / off, and
    beside them the moments step's FIRST frame, which stages its tile in every workgroup too.
(b) Quality.  Per frame, MSE against the --ref-spp frame of the moments step alone and of the step + `run_guided`, on one-chunk
    frames, OFF against VARIANCE with gamma 0.5, 1, 2 and +inf (which must equal OFF), in both background modes — over the whole
    frame, and split into the background pixels' and the hit pixels' parts of it — and the share of pixels clipped.
    --motion, --pan and --config as for --cubic.

    python tools/temporal_bench.py --clip [--config 3] [--motion pan|orbit] [--pan 2.5] [--cost-only] [the switches above]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from rayz_amd import capi, render, tracer  # noqa: E402

STEP_BYTES = 52 + 64 + 88  # per pixel: what a step must read and write (module docstring)
MOMENTS_STEP_BYTES = 40 + 64 + 104  # .. and a moments step
FEEDBACK_STEP_BYTES = MOMENTS_STEP_BYTES + 16  # .. and a feedback step: the m1 record in
FEEDBACK_WRITE_BYTES = 12 + 16 + 16  # the write kernel: the image and the colour record in, the record out


def panned(cam, pixels):
    c = capi.CameraDesc.from_buffer_copy(cam)
    for j in range(3):
        c.px_origin[j] = cam.px_origin[j] + pixels * cam.px_du[j]
    return c


def copy_ms(n_bytes, reps, warmup):
    """Median [min, max] of an event-bracketed device copy of n_bytes (read) to n_bytes (written)."""
    src = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    dst = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    for _ in range(warmup):
        dst.copy_(src)
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main_moments(args):
    """--moments: see the module docstring."""
    render.init(0)
    t = tracer.randomBouncing(args.width, -50, 50, seed=42)  # config 3
    t.samples_per_px, t.max_bounces = args.spp, 50
    t.set_gpu(render_seed=1, traversal=capi.TRAVERSAL_BVH, chunk_spp=0)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    p.tmin = 1e-3
    w, h = p.width, p.height
    n = w * h
    assert args.spp % 2 == 0 and args.spp <= 16, "--moments wants an even spp of at most 16: one automatic chunk, two tracked ones"
    ds = render.DeviceScene(sd)
    res = {"mode": "moments", "size": f"{w}x{h}", "frames": args.frames, "pan_px": args.pan, "spp": args.spp, "ref_spp": args.ref_spp,
           "reps": args.reps, "settle": args.settle, "step_bytes_per_pixel": STEP_BYTES, "moments_step_bytes_per_pixel": MOMENTS_STEP_BYTES}
    seq = []
    for k in range(args.frames):
        c = panned(cam, args.pan * k)
        q = capi.RenderParams.from_buffer_copy(p)
        q.seed, q.chunk_spp = 1000 + k, 0
        one = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")  # the frame in ONE chunk: no variance to be had
        torch.cuda.synchronize()
        ds.render_into(c, q, one.data_ptr())
        ds.sync()
        q.chunk_spp = args.spp // 2
        pr = ds.progressive(c, q, track_noise=True)  # the same seed in two chunks, tracked: another summation tree, and a variance
        two = torch.empty_like(one)
        torch.cuda.synchronize()
        while not pr.done:
            pr.step(0, two.data_ptr())
        assert pr.chunks_done == 2
        var = pr.noise_rgb()
        pr.stats()
        pr.close()
        g = ds.gbuffer(c, p)
        ds.query_sync()
        q.samples_per_px, q.chunk_spp, q.seed = args.ref_spp, 0, 7
        ref = torch.empty_like(one)
        torch.cuda.synchronize()
        ds.render_into(c, q, ref.data_ptr())
        ds.sync()
        seq.append((c, one, two, var, g, ref))
        print(f"frame {k}: {args.spp} spp in one chunk and in two, reference {args.ref_spp} spp", flush=True)
    mse = lambda a, ref: float(((a.double() - ref.double()) ** 2).mean())  # noqa: E731

    # ---- (a) cost -------------------------------------------------------------------------------------------------------------
    res["copy"] = {}
    for name, nbytes in (("plain", STEP_BYTES), ("moments", MOMENTS_STEP_BYTES)):
        cp = copy_ms(n * nbytes // 2, args.reps, args.warmup)
        res["copy"][name] = {"ms": cp[0], "min": cp[1], "max": cp[2]}
        print(f"copy moving a {name} step's compulsory bytes ({n * nbytes / 1e6:.1f} MB read + written): {cp[0]:.4f} ms [{cp[1]:.4f}, {cp[2]:.4f}] "
              f"({n * nbytes / cp[0] / 1e9:.2f} TB/s)", flush=True)
    plain, mom = render.Temporal(w, h), render.Temporal(w, h, moments=True)
    out, vout = torch.empty((h, w, 3), dtype=torch.float32, device="cuda"), torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    length, w2 = torch.empty((h, w), dtype=torch.float32, device="cuda"), torch.empty((h, w), dtype=torch.float32, device="cuda")

    def plain_step(s):
        plain.step(s[2], s[3], s[4], s[0], args.spp, out=out, var_out=vout, length=length)

    def moments_step(s, **prm):
        mom.step_moments(s[1], s[4], s[0], args.spp, out=out, var_out=vout, length=length, w2=w2, **prm)

    # (state, steps before the timed one, the timed frame)
    states = [("first", 0, 0), ("static-second", 1, 0), ("static-settled", args.settle, 0), ("panned-settled", args.settle, 1)]
    res["cost"] = {}
    for what, before, last in states:
        row = {}
        for name, tm, step, nbytes in (("plain", plain, plain_step, STEP_BYTES), ("moments", mom, moments_step, MOMENTS_STEP_BYTES)):
            ms = []
            for r in range(args.warmup + args.reps):
                tm.reset()
                for _ in range(before):
                    step(seq[0])
                step(seq[last])
                x = tm.timing()
                if r >= args.warmup:
                    ms.append(x)
            med = statistics.median(ms)
            cpm = res["copy"][name]["ms"]
            row[name] = {"ms": med, "min": min(ms), "max": max(ms), "ratio_to_copy": med / cpm}
            print(f"{name:7s} step, {what:14s}: {med:.4f} ms [{min(ms):.4f}, {max(ms):.4f}] = {med / cpm:.2f} x the copy of its compulsory bytes "
                  f"({n * nbytes / med / 1e9:.2f} TB/s of them)", flush=True)
        if what != "first":
            torch.cuda.synchronize()
            hit = seq[last][4].index >= 0
            row["share_spatial"] = float((w2[hit] > capi.TEMPORAL_MOMENTS_DEFAULTS["w2_max"]).float().mean())
            print(f"        {what}: {row['share_spatial']:.4f} of the hit pixels took the spatial estimate", flush=True)
        row["moments_over_plain"] = row["moments"]["ms"] / row["plain"]["ms"]
        res["cost"][what] = row

    # ---- (b) quality at the defaults; (c) the sweep ------------------------------------------------------------------------------
    dn = render.Denoiser(w, h)
    den = torch.empty_like(out)
    plain.reset()
    rows = []
    for k, s in enumerate(seq):
        plain_step(s)
        dn.run_guided(out, vout, s[4], out=den)
        torch.cuda.synchronize()
        rows.append({"frame": k, "mse_raw": mse(s[1], s[5]), "mse_raw_two_chunks": mse(s[2], s[5]), "mse_plain": mse(out, s[5]),
                     "mse_plain_guided": mse(den, s[5])})

    def run(**prm):
        mom.reset()
        got = []
        for k, s in enumerate(seq):
            moments_step(s, **prm)
            dn.run_guided(out, vout, s[4], out=den)
            torch.cuda.synchronize()
            hit = s[4].index >= 0
            wm = prm.get("w2_max", capi.TEMPORAL_MOMENTS_DEFAULTS["w2_max"])
            got.append({"mse_moments": mse(out, s[5]), "mse_moments_guided": mse(den, s[5]),
                        "share_spatial": float((w2[hit] > wm).float().mean()) if bool(hit.any()) else 0.0})
        return got

    for row, m in zip(rows, run()):
        row.update(m)
        r = row["mse_raw"]
        print(f"frame {row['frame']:2d}: MSE raw (one chunk) {r:.4e}; plain step on the two-chunk frame x{row['mse_plain'] / r:.4f}, + guided "
              f"x{row['mse_plain_guided'] / r:.4f}; moments step x{row['mse_moments'] / r:.4f}, + guided x{row['mse_moments_guided'] / r:.4f}; "
              f"{row['share_spatial']:.4f} of the hit pixels took the spatial estimate", flush=True)
    res["defaults"] = {"params": {**capi.TEMPORAL_DEFAULTS, **capi.TEMPORAL_MOMENTS_DEFAULTS}, "rows": rows}
    res["sweep"] = []
    for wm in (0.0, 0.125, 0.25, 0.5, 1.0):
        for mt in (2.0, 4.0, 9.0, 16.0, 25.0):
            got = run(w2_max=wm, min_taps=mt)
            ratio = [g["mse_moments_guided"] / r["mse_raw"] for g, r in zip(got, rows)]
            row = {"w2_max": wm, "min_taps": mt, "first": ratio[0], "second": ratio[1], "mean_later": statistics.mean(ratio[1:]), "last": ratio[-1],
                   "share_spatial_later": statistics.mean(g["share_spatial"] for g in got[1:])}
            res["sweep"].append(row)
            print(f"  w2_max {wm:g} min_taps {mt:g}: moments + guided MSE / raw: first frame {row['first']:.4f}, second {row['second']:.4f}, mean over "
                  f"frames 1.. {row['mean_later']:.4f}, last {row['last']:.4f}; spatial share on frames 1.. {row['share_spatial_later']:.4f}", flush=True)
    plain.close()
    mom.close()
    dn.close()
    ds.close()
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


def main_counts(args):
    """--counts: see the module docstring."""
    render.init(0)
    t = tracer.randomBouncing(args.width, -50, 50, seed=42)  # config 3
    t.samples_per_px, t.max_bounces = 16, 50
    t.set_gpu(render_seed=1, traversal=capi.TRAVERSAL_BVH, chunk_spp=0)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    p.tmin = 1e-3
    w, h = p.width, p.height
    n, f = w * h, 2
    ds = render.DeviceScene(sd)
    res = {"mode": "counts", "size": f"{w}x{h}", "frames": args.frames, "pan_px": args.pan, "lattice_spp": 16, "factor": f,
           "ref_spp": args.ref_spp, "reps": args.reps}
    phases = render.phase_sequence(f)
    up = render.Upscaler(w, h, f)
    mse = lambda a, ref: float(((a.double() - ref.double()) ** 2).mean())  # noqa: E731

    def params(spp, seed, chunk=0, base=p):
        q = capi.RenderParams.from_buffer_copy(base)
        q.samples_per_px, q.seed, q.chunk_spp = spp, seed, chunk
        return q

    def whole(c, q):
        frame = torch.empty((q.height, q.width, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ds.render_into(c, q, frame.data_ptr())
        ds.sync()
        return frame

    seq = []
    for k in range(args.frames):
        c = panned(cam, args.pan * k)
        g = ds.gbuffer(c, p)
        ds.query_sync()
        phase = phases[k % len(phases)]
        pixels, dest = render.lattice_pixels(w, h, f, phase, device="cuda")
        lat = torch.full((h // f, w // f, 3), float("nan"), dtype=torch.float32, device="cuda")
        ds.render_pixels(c, params(16, 1000 + k), pixels, dest=dest, out=lat)
        ds.sync()
        rebuilt = up.run(lat, g.lattice(f, phase), g, phase=phase)  # the lattice's pixels as they are, the others around them
        counts = render.lattice_counts(w, h, f, phase, 16, device="cuda")
        c_lo, p_lo = render.lowres_camera(c, f), render.lowres_params(p, f)
        pr = ds.progressive(c_lo, params(16, 1000 + k, 8, p_lo), track_noise=True)
        lo = torch.empty((h // f, w // f, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        while not pr.done:
            pr.step(0, lo.data_ptr())
        lo_var = pr.noise_rgb()
        pr.stats()
        pr.close()
        g_lo = ds.gbuffer(c_lo, p_lo)
        ds.query_sync()
        four = whole(c, params(4, 1000 + k))
        ref = whole(c, params(args.ref_spp, 7))
        torch.cuda.synchronize()
        seq.append(dict(cam=c, g=g, phase=phase, rebuilt=rebuilt, counts=counts, lo=lo, lo_var=lo_var, g_lo=g_lo, four=four, ref=ref))
        print(f"frame {k}: phase {phase}, lattice 16 spp, low resolution 16 spp, full 4 spp, reference {args.ref_spp} spp", flush=True)

    # ---- (a) cost -------------------------------------------------------------------------------------------------------------
    out, vout = torch.empty((h, w, 3), dtype=torch.float32, device="cuda"), torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    length, w2 = torch.empty((h, w), dtype=torch.float32, device="cuda"), torch.empty((h, w), dtype=torch.float32, device="cuda")
    var_in = torch.full((h, w, 3), 0.01, dtype=torch.float32, device="cuda")
    plain, mom = render.Temporal(w, h), render.Temporal(w, h, moments=True)
    sixteen = torch.full((h, w), 16, dtype=torch.int32, device="cuda")

    def step(kind, s, spp):
        if kind.startswith("plain"):
            plain.step(s["rebuilt"], var_in, s["g"], s["cam"], spp, out=out, var_out=vout, length=length)
        else:
            mom.step_moments(s["rebuilt"], s["g"], s["cam"], spp, out=out, var_out=vout, length=length, w2=w2)

    res["copy"], res["cost"] = {}, {}
    kinds = [("plain", STEP_BYTES, False), ("plain counts", STEP_BYTES + 4, True), ("moments", MOMENTS_STEP_BYTES, False),
             ("moments counts", MOMENTS_STEP_BYTES + 4, True)]
    for name, nbytes, _ in kinds:
        cp = copy_ms(n * nbytes // 2, args.reps, args.warmup)
        res["copy"][name] = {"ms": cp[0], "min": cp[1], "max": cp[2]}
        print(f"copy moving a {name} step's compulsory bytes ({n * nbytes / 1e6:.1f} MB read + written): {cp[0]:.4f} ms [{cp[1]:.4f}, {cp[2]:.4f}]",
              flush=True)
    for what, last in (("first", None), ("static", 0), ("panned", 1)):
        row = {}
        for name, nbytes, counted in kinds:
            tm = plain if name.startswith("plain") else mom
            ms = []
            for r in range(args.warmup + args.reps):
                tm.reset()
                # (the history behind a timed step is a full one: every record holds samples, as after a phase cycle)
                step(name, seq[0], sixteen if counted else 16)
                if last is not None:
                    step(name, seq[last], seq[last]["counts"] if counted else 16)
                x = tm.timing()
                if r >= args.warmup:
                    ms.append(x)
            med, cpm = statistics.median(ms), res["copy"][name]["ms"]
            row[name] = {"ms": med, "min": min(ms), "max": max(ms), "ratio_to_copy": med / cpm}
            print(f"{name:14s} step, {what:6s}: {med:.4f} ms [{min(ms):.4f}, {max(ms):.4f}] = {med / cpm:.2f} x the copy of its compulsory bytes",
                  flush=True)
        row["plain_counts_over_plain"] = row["plain counts"]["ms"] / row["plain"]["ms"]
        row["moments_counts_over_moments"] = row["moments counts"]["ms"] / row["moments"]["ms"]
        print(f"        {what}: counts / scalar: plain {row['plain_counts_over_plain']:.3f}, moments {row['moments_counts_over_moments']:.3f}", flush=True)
        res["cost"][what] = row

    # ---- (b) quality at the defaults ------------------------------------------------------------------------------------------------
    dn = render.Denoiser(w, h)
    den = torch.empty_like(out)
    full = render.Temporal(w, h, moments=True)
    mom.reset()
    rows = []
    for k, s in enumerate(seq):
        row = {"frame": k, "mse_four_raw": mse(s["four"], s["ref"])}
        mom.step_moments(s["rebuilt"], s["g"], s["cam"], s["counts"], out=out, var_out=vout, length=length)
        dn.run_guided(out, vout, s["g"], out=den)
        torch.cuda.synchronize()
        hit = s["g"].index >= 0
        row.update(mse_lattice=mse(out, s["ref"]), mse_lattice_guided=mse(den, s["ref"]),
                   lattice_sampled_share=float((length[hit] > 0).float().mean()))
        up_c, var_c = up.run(s["lo"], s["g_lo"], s["g"], var_rgb=s["lo_var"])
        dn.run_guided(up_c, var_c, s["g"], out=den)
        torch.cuda.synchronize()
        row.update(mse_lowres=mse(up_c, s["ref"]), mse_lowres_guided=mse(den, s["ref"]))
        full.step_moments(s["four"], s["g"], s["cam"], 4, out=out, var_out=vout)
        dn.run_guided(out, vout, s["g"], out=den)
        torch.cuda.synchronize()
        row.update(mse_full4=mse(out, s["ref"]), mse_full4_guided=mse(den, s["ref"]))
        rows.append(row)
        print(f"frame {k:2d}: MSE lattice + counts step {row['mse_lattice']:.4e}, + guided {row['mse_lattice_guided']:.4e} "
              f"({row['lattice_sampled_share']:.4f} of the hit pixels hold samples); low resolution + upscale {row['mse_lowres']:.4e}, + guided "
              f"{row['mse_lowres_guided']:.4e}; full 4 spp + moments step {row['mse_full4']:.4e}, + guided {row['mse_full4_guided']:.4e}", flush=True)
    res["rows"] = rows
    for key in ("mse_lattice_guided", "mse_lowres_guided", "mse_full4_guided"):
        res["mean_" + key] = statistics.mean(r[key] for r in rows)
        print(f"mean over the frames of {key}: {res['mean_' + key]:.4e}", flush=True)
    plain.close(), mom.close(), full.close(), dn.close(), up.close(), ds.close()
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump(res, fh, indent=1)


def event_ms(fn, reps, warmup):
    """Median [min, max] of fn() between two events on torch's current stream (fn enqueues there)."""
    ms = []
    for r in range(warmup + reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        if r >= warmup:
            ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main_feedback(args):
    """--feedback: see the module docstring."""
    render.init(0)
    t = tracer.randomBouncing(args.width, -50, 50, seed=42)  # config 3
    t.samples_per_px, t.max_bounces = args.spp, 50
    t.set_gpu(render_seed=1, traversal=capi.TRAVERSAL_BVH, chunk_spp=0)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    p.tmin = 1e-3
    w, h = p.width, p.height
    n = w * h
    assert args.spp <= 16, "--feedback wants an spp of at most 16: one automatic chunk"
    ds = render.DeviceScene(sd)
    res = {"mode": "feedback", "size": f"{w}x{h}", "frames": args.frames, "pan_px": args.pan, "spp": args.spp, "ref_spp": args.ref_spp,
           "reps": args.reps, "settle": args.settle, "moments_step_bytes_per_pixel": MOMENTS_STEP_BYTES,
           "feedback_step_bytes_per_pixel": FEEDBACK_STEP_BYTES, "feedback_write_bytes_per_pixel": FEEDBACK_WRITE_BYTES}
    seq = []
    for k in range(args.frames):
        c = panned(cam, args.pan * k)
        q = capi.RenderParams.from_buffer_copy(p)
        q.seed, q.chunk_spp = 1000 + k, 0
        one = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ds.render_into(c, q, one.data_ptr())
        ds.sync()
        g = ds.gbuffer(c, p)
        ds.query_sync()
        q.samples_per_px, q.seed = args.ref_spp, 7
        ref = torch.empty_like(one)
        torch.cuda.synchronize()
        ds.render_into(c, q, ref.data_ptr())
        ds.sync()
        seq.append((c, one, g, ref))
        print(f"frame {k}: {args.spp} spp in one chunk, reference {args.ref_spp} spp", flush=True)
    mse = lambda a, ref: float(((a.double() - ref.double()) ** 2).mean())  # noqa: E731

    # ---- (a) cost -------------------------------------------------------------------------------------------------------------
    res["copy"] = {}
    for name, nbytes in (("moments", MOMENTS_STEP_BYTES), ("feedback", FEEDBACK_STEP_BYTES), ("write", FEEDBACK_WRITE_BYTES)):
        cp = copy_ms(n * nbytes // 2, args.reps, args.warmup)
        res["copy"][name] = {"ms": cp[0], "min": cp[1], "max": cp[2]}
        print(f"copy moving the compulsory bytes of a {name} ({n * nbytes / 1e6:.1f} MB read + written): {cp[0]:.4f} ms [{cp[1]:.4f}, {cp[2]:.4f}] "
              f"({n * nbytes / cp[0] / 1e9:.2f} TB/s)", flush=True)
    mom, fbk = render.Temporal(w, h, moments=True), render.Temporal(w, h, moments=True, feedback=True)
    out, vout = torch.empty((h, w, 3), dtype=torch.float32, device="cuda"), torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    length, w2 = torch.empty((h, w), dtype=torch.float32, device="cuda"), torch.empty((h, w), dtype=torch.float32, device="cuda")

    def step(tm, s):
        tm.step_moments(s[1], s[2], s[0], args.spp, out=out, var_out=vout, length=length, w2=w2)

    states = [("first", 0, 0), ("static-second", 1, 0), ("static-settled", args.settle, 0), ("panned-settled", args.settle, 1)]
    res["cost"] = {}
    for what, before, last in states:
        row = {}
        for name, tm, nbytes in (("moments", mom, MOMENTS_STEP_BYTES), ("feedback", fbk, FEEDBACK_STEP_BYTES)):
            ms = []
            for r in range(args.warmup + args.reps):
                tm.reset()
                for _ in range(before):
                    step(tm, seq[0])
                step(tm, seq[last])
                x = tm.timing()
                if r >= args.warmup:
                    ms.append(x)
            med = statistics.median(ms)
            cpm = res["copy"][name]["ms"]
            row[name] = {"ms": med, "min": min(ms), "max": max(ms), "ratio_to_copy": med / cpm}
            print(f"{name:8s} step, {what:14s}: {med:.4f} ms [{min(ms):.4f}, {max(ms):.4f}] = {med / cpm:.2f} x the copy of its compulsory bytes "
                  f"({n * nbytes / med / 1e9:.2f} TB/s of them)", flush=True)
        row["feedback_over_moments"] = row["feedback"]["ms"] / row["moments"]["ms"]
        res["cost"][what] = row
    torch.cuda.synchronize()
    side = torch.cuda.Stream()  # (a stream of torch's own: its events bracket what the library enqueues there)
    with torch.cuda.stream(side):
        wr = event_ms(lambda: fbk.feedback(out, stream=side.cuda_stream), args.reps, args.warmup)
    torch.cuda.synchronize()
    cpm = res["copy"]["write"]["ms"]
    res["cost"]["write"] = {"ms": wr[0], "min": wr[1], "max": wr[2], "ratio_to_copy": wr[0] / cpm}
    print(f"feedback write: {wr[0]:.4f} ms [{wr[1]:.4f}, {wr[2]:.4f}] = {wr[0] / cpm:.2f} x the copy of its compulsory bytes "
          f"({n * FEEDBACK_WRITE_BYTES / wr[0] / 1e9:.2f} TB/s of them)", flush=True)
    dn = render.Denoiser(w, h)
    den, tap = torch.empty_like(out), torch.empty_like(out)
    s0 = seq[0]
    step(mom, s0)
    runs = {}
    for name, kw in (("untapped", {}), ("tapped", dict(tap_level=1, tap_out=tap))):
        ms = []
        for r in range(args.warmup + args.reps):
            dn.run_guided(out, vout, s0[2], out=den, **kw)
            pack, levels = dn.timing()
            if r >= args.warmup:
                ms.append((pack + sum(levels), levels[0]))
        tot, l0 = [m[0] for m in ms], [m[1] for m in ms]
        runs[name] = {"ms": statistics.median(tot), "min": min(tot), "max": max(tot), "level0_ms": statistics.median(l0)}
        print(f"run_guided, {name:8s}: {runs[name]['ms']:.4f} ms [{min(tot):.4f}, {max(tot):.4f}] (pack pass + levels), level 0 alone "
              f"{runs[name]['level0_ms']:.4f} ms", flush=True)
    runs["tapped_over_untapped"] = runs["tapped"]["ms"] / runs["untapped"]["ms"]
    res["cost"]["run_guided"] = runs

    # ---- (b) quality at the defaults -----------------------------------------------------------------------------------------------
    mom.reset(), fbk.reset()
    rows = []
    for k, s in enumerate(seq):
        step(mom, s)
        dn.run_guided(out, vout, s[2], out=den)
        torch.cuda.synchronize()
        row = {"frame": k, "mse_raw": mse(s[1], s[3]), "mse_moments": mse(out, s[3]), "mse_moments_guided": mse(den, s[3])}
        step(fbk, s)
        dn.run_guided(out, vout, s[2], out=den, tap_level=1, tap_out=tap)
        fbk.feedback(tap)
        torch.cuda.synchronize()
        row.update({"mse_feedback": mse(out, s[3]), "mse_feedback_guided": mse(den, s[3])})
        rows.append(row)
        r = row["mse_raw"]
        print(f"frame {k:2d}: MSE raw (one chunk) {r:.4e}; moments step x{row['mse_moments'] / r:.4f}, + guided x{row['mse_moments_guided'] / r:.4f}; "
              f"with the level-1 tap fed back: step x{row['mse_feedback'] / r:.4f}, + guided x{row['mse_feedback_guided'] / r:.4f}", flush=True)
    res["defaults"] = {"params": {**capi.TEMPORAL_DEFAULTS, **capi.TEMPORAL_MOMENTS_DEFAULTS}, "rows": rows}
    mom.close(), fbk.close(), dn.close(), ds.close()
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


def orbited(cam, pixels, width, height):
    """`cam` turned about the centre of its pixel plane (the focus point), around the image's vertical axis, so that look_from
    moves along its arc by `pixels` pixel widths as measured in that plane: look_from AND the view direction change, a point in the
    focus plane stays where it is, nearer and farther ones move in opposite directions by amounts that depend on their depth."""
    import numpy as np

    lf, du, dv, po = (np.array(list(getattr(cam, k))) for k in ("look_from", "px_du", "px_dv", "px_origin"))
    pivot = po + du * (width / 2) + dv * (height / 2)
    axis = dv / np.linalg.norm(dv)
    th = pixels * np.linalg.norm(du) / np.linalg.norm(pivot - lf)

    def rot(v):  # Rodrigues
        return v * np.cos(th) + np.cross(axis, v) * np.sin(th) + axis * (axis @ v) * (1 - np.cos(th))

    c = capi.CameraDesc.from_buffer_copy(cam)
    nlf = pivot + rot(lf - pivot)
    npo = pivot + rot(po - pivot)
    for name, v in (("look_from", nlf), ("px_origin", npo), ("px_du", rot(du)), ("px_dv", rot(dv)),
                    ("defocus_u", rot(np.array(list(cam.defocus_u)))), ("defocus_v", rot(np.array(list(cam.defocus_v))))):
        for j in range(3):
            getattr(c, name)[j] = float(v[j])
    return c


def main_cubic(args):
    """--cubic: see the module docstring."""
    if args.lib:  # an older build: without the mode's two entry points
        capi.PROTOTYPES[:] = [q for q in capi.PROTOTYPES if "resampling" not in q[0]]
        capi.LIB_PATH = os.path.abspath(args.lib)
    render.init(0)
    t = tracer.randomBouncing(args.width, seed=42) if args.config == 2 else tracer.randomBouncing(args.width, -50, 50, seed=42)
    t.samples_per_px, t.max_bounces = args.spp, 50
    t.set_gpu(render_seed=1, traversal=capi.TRAVERSAL_BVH, chunk_spp=0)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    p.tmin = 1e-3
    w, h = p.width, p.height
    n = w * h
    assert args.spp <= 16, "--cubic wants an spp of at most 16: one automatic chunk"
    ds = render.DeviceScene(sd)
    has_mode = any(name == "rayz_hip_temporal_set_resampling" for name, _, _ in capi.PROTOTYPES) and not args.lib
    move = (lambda k: orbited(cam, args.pan * k, w, h)) if args.motion == "orbit" else (lambda k: panned(cam, args.pan * k))
    res = {"mode": "cubic", "config": args.config, "motion": args.motion, "size": f"{w}x{h}", "frames": args.frames, "px_per_frame": args.pan,
           "spp": args.spp, "ref_spp": args.ref_spp, "reps": args.reps, "build": args.lib_label or ("--lib" if args.lib else "this build")}
    kinds = torch.tensor([sd.materials[i].kind for i in range(sd.n_materials)], device="cuda")
    seq = []
    for k in range(args.frames if not args.cost_only else 2):
        c = move(k)
        q = capi.RenderParams.from_buffer_copy(p)
        q.seed, q.chunk_spp = 1000 + k, 0
        one = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ds.render_into(c, q, one.data_ptr())
        ds.sync()
        g = ds.gbuffer(c, p)
        ds.query_sync()
        ref = None
        if not args.cost_only:
            q.samples_per_px, q.seed = args.ref_spp, 7
            ref = torch.empty_like(one)
            torch.cuda.synchronize()
            ds.render_into(c, q, ref.data_ptr())
            ds.sync()
        seq.append((c, one, g, ref))
        print(f"frame {k}: {args.spp} spp in one chunk" + ("" if ref is None else f", reference {args.ref_spp} spp"), flush=True)
    var = torch.full((h, w, 3), 1e-3, dtype=torch.float32, device="cuda")  # (the plain step's cost does not depend on the variance's values)
    out, vout = torch.empty((h, w, 3), dtype=torch.float32, device="cuda"), torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    taken = torch.zeros((h, w), dtype=torch.uint8, device="cuda")

    # ---- (a) cost: the moved step, the variants alternating -------------------------------------------------------------------
    res["cost"] = {}
    modes = ("bilinear", "cubic") if has_mode else ("bilinear",)
    handles = {(kind, mode): render.Temporal(w, h, moments=kind == "moments") for kind in ("plain", "moments") for mode in modes}
    for (kind, mode), tm in handles.items():
        if has_mode:
            tm.set_resampling(mode, taken=taken if mode == "cubic" else False)

    def two_steps(kind, tm):
        tm.reset()
        for c, one, g, _ in seq[:2]:
            if kind == "plain":
                tm.step(one, var, g, c, args.spp, out=out, var_out=vout)
            else:
                tm.step_moments(one, g, c, args.spp, out=out, var_out=vout)

    ms = {k: [] for k in handles}
    for r in range(args.warmup + args.reps):
        for (kind, mode), tm in handles.items():
            two_steps(kind, tm)
            x = tm.timing()
            if r >= args.warmup:
                ms[(kind, mode)].append(x)
    for kind, nbytes in (("plain", STEP_BYTES), ("moments", MOMENTS_STEP_BYTES)):
        for mode in modes:
            per_pixel = nbytes + (1 if mode == "cubic" else 0)  # (the cubic handles here write the taken bytes)
            cp = copy_ms(n * per_pixel // 2, args.reps, args.warmup)
            v = ms[(kind, mode)]
            med = statistics.median(v)
            share = None
            if mode == "cubic":
                two_steps(kind, handles[(kind, mode)])
                torch.cuda.synchronize()
                share = float(taken[seq[1][2].index >= 0].float().mean())
            res["cost"][f"{kind} {mode}"] = {"ms": med, "min": min(v), "max": max(v), "bytes_per_pixel": per_pixel, "copy_ms": cp[0], "copy_min": cp[1],
                                             "copy_max": cp[2], "ratio_to_copy": med / cp[0], "taken_share_of_hits": share}
            print(f"{kind} step, {mode:8s}, {args.motion} {args.pan} px: {med:.4f} ms [{min(v):.4f}, {max(v):.4f}] = {med / cp[0]:.2f} x the copy of its "
                  f"{per_pixel} B per pixel ({cp[0]:.4f} ms [{cp[1]:.4f}, {cp[2]:.4f}])"
                  + ("" if share is None else f"; {share:.4f} of the hit pixels took the sixteen taps"), flush=True)
    for tm in handles.values():
        tm.close()

    # ---- (b) quality: moments handles on the one-chunk frames -------------------------------------------------------------------
    if not args.cost_only and has_mode:
        dn = render.Denoiser(w, h)
        den = torch.empty_like(out)
        res["rows"] = []
        tms = {mode: render.Temporal(w, h, moments=True, resampling=mode) for mode in modes}
        tms["cubic"].set_resampling("cubic", taken=taken)
        for k, (c, one, g, ref) in enumerate(seq):
            hit = g.index >= 0
            spec = hit & (kinds[g.material.clamp(min=0).long()] != capi.MAT_DIFFUSE)  # first hit metal or glass, as denoise_bench.py --chain
            diff = hit & ~spec

            def mse3(a):
                err = ((a.double() - ref.double()) ** 2).mean(dim=2)
                return [float(err.mean()), float(err[diff].mean()), float(err[spec].mean())]

            row = {"frame": k, "raw": mse3(one), "share_diffuse": float(diff.float().mean()), "share_specular": float(spec.float().mean())}
            for mode, tm in tms.items():
                tm.step_moments(one, g, c, args.spp, out=out, var_out=vout)
                dn.run_guided(out, vout, g, out=den)
                torch.cuda.synchronize()
                row[f"temporal_{mode}"], row[f"temporal_guided_{mode}"] = mse3(out), mse3(den)
            row["taken_share_of_hits"] = float(taken[hit].float().mean())
            res["rows"].append(row)
            rel = lambda key: " ".join(f"{a / b:.4f}" for a, b in zip(row[key], row["raw"]))  # noqa: E731
            print(f"frame {k:2d}: MSE / raw (all | diffuse | metal or glass): temporal bilinear {rel('temporal_bilinear')}, cubic {rel('temporal_cubic')}; "
                  f"+ guided bilinear {rel('temporal_guided_bilinear')}, cubic {rel('temporal_guided_cubic')}; taken {row['taken_share_of_hits']:.4f}", flush=True)
        print(f"raw MSE of the last frame (all | diffuse | metal or glass): {row['raw']}; pixel shares: diffuse {row['share_diffuse']:.3f}, "
              f"metal or glass {row['share_specular']:.3f}", flush=True)
        for tm in tms.values():
            tm.close()
        dn.close()
    ds.close()
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


def main_background(args):
    """--background: see the module docstring."""
    render.init(0)
    t = tracer.randomBouncing(args.width, seed=42) if args.config == 2 else tracer.randomBouncing(args.width, -50, 50, seed=42)
    t.samples_per_px, t.max_bounces = args.spp, 50
    t.set_gpu(render_seed=1, traversal=capi.TRAVERSAL_BVH, chunk_spp=0)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    p.tmin = 1e-3
    w, h = p.width, p.height
    n = w * h
    assert args.spp <= 16, "--background wants an spp of at most 16: one automatic chunk"
    ds = render.DeviceScene(sd)
    move = (lambda k: orbited(cam, args.pan * k, w, h)) if args.motion == "orbit" else (lambda k: panned(cam, args.pan * k))
    res = {"mode": "background", "config": args.config, "motion": args.motion, "size": f"{w}x{h}", "frames": args.frames,
           "px_per_frame": args.pan, "spp": args.spp, "ref_spp": args.ref_spp, "reps": args.reps}
    seq = []
    for k in range(args.frames if not args.cost_only else 2):
        c = move(k)
        q = capi.RenderParams.from_buffer_copy(p)
        q.seed, q.chunk_spp = 1000 + k, 0
        one = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ds.render_into(c, q, one.data_ptr())
        ds.sync()
        g = ds.gbuffer(c, p)
        ds.query_sync()
        ref = None
        if not args.cost_only:
            q.samples_per_px, q.seed = args.ref_spp, 7
            ref = torch.empty_like(one)
            torch.cuda.synchronize()
            ds.render_into(c, q, ref.data_ptr())
            ds.sync()
        seq.append((c, one, g, ref))
        print(f"frame {k}: {args.spp} spp in one chunk, background {float((g.index < 0).float().mean()):.4f} of the pixels"
              + ("" if ref is None else f", reference {args.ref_spp} spp"), flush=True)
    var = torch.full((h, w, 3), 1e-3, dtype=torch.float32, device="cuda")  # (the plain step's cost does not depend on the variance's values)
    out, vout = torch.empty((h, w, 3), dtype=torch.float32, device="cuda"), torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    length = torch.empty((h, w), dtype=torch.float32, device="cuda")

    # ---- (a) cost: first, static and moved, the two modes alternating ------------------------------------------------------------
    res["cost"] = {}
    modes = ("input", "accumulate")
    handles = {(kind, mode): render.Temporal(w, h, moments=kind == "moments", background=mode) for kind in ("plain", "moments") for mode in modes}

    def steps(kind, tm, what):
        tm.reset()
        for c, one, g, _ in {"first": seq[:1], "static": [seq[0], seq[0]], "moved": seq[:2]}[what]:
            if kind == "plain":
                tm.step(one, var, g, c, args.spp, out=out, var_out=vout)
            else:
                tm.step_moments(one, g, c, args.spp, out=out, var_out=vout)

    for what in ("first", "static", "moved"):
        ms = {k: [] for k in handles}
        for r in range(args.warmup + args.reps):
            for (kind, mode), tm in handles.items():
                steps(kind, tm, what)
                x = tm.timing()
                if r >= args.warmup:
                    ms[(kind, mode)].append(x)
        for kind, nbytes in (("plain", STEP_BYTES), ("moments", MOMENTS_STEP_BYTES)):
            cp = copy_ms(n * nbytes // 2, args.reps, args.warmup)
            med = {mode: statistics.median(ms[(kind, mode)]) for mode in modes}
            for mode in modes:
                v = ms[(kind, mode)]
                res["cost"][f"{kind} {what} {mode}"] = {"ms": med[mode], "min": min(v), "max": max(v), "bytes_per_pixel": nbytes, "copy_ms": cp[0],
                                                        "copy_min": cp[1], "copy_max": cp[2], "ratio_to_copy": med[mode] / cp[0],
                                                        "ratio_to_input": med[mode] / med["input"]}
                print(f"{kind:7s} step, {what:6s}, {mode:10s}: {med[mode]:.4f} ms [{min(v):.4f}, {max(v):.4f}] = {med[mode] / cp[0]:.2f} x the copy of "
                      f"its {nbytes} B per pixel ({cp[0]:.4f} ms [{cp[1]:.4f}, {cp[2]:.4f}]), {med[mode] / med['input']:.3f} x the input mode", flush=True)
    for tm in handles.values():
        tm.close()

    # ---- (b) quality: moments handles on the one-chunk frames ---------------------------------------------------------------------
    if not args.cost_only:
        dn = render.Denoiser(w, h)
        den = torch.empty_like(out)
        res["rows"] = []
        tms = {mode: render.Temporal(w, h, moments=True, background=mode) for mode in modes}
        for k, (c, one, g, ref) in enumerate(seq):
            bg = g.index < 0

            def mse2(a):
                err = ((a.double() - ref.double()) ** 2).mean(dim=2)
                return [float(err.mean()), float(err[bg].mean()) if bool(bg.any()) else 0.0, float(err[~bg].mean())]

            row = {"frame": k, "raw": mse2(one), "share_background": float(bg.float().mean())}
            for mode, tm in tms.items():
                tm.step_moments(one, g, c, args.spp, out=out, var_out=vout, length=length)
                dn.run_guided(out, vout, g, out=den)
                torch.cuda.synchronize()
                row[f"temporal_{mode}"], row[f"temporal_guided_{mode}"] = mse2(out), mse2(den)
                if mode == "accumulate":
                    row["background_found"] = float((length[bg] > args.spp).float().mean()) if bool(bg.any()) else 0.0
                    row["background_mean_length"] = float(length[bg].mean()) if bool(bg.any()) else 0.0
            res["rows"].append(row)
            whole = row["raw"][0]  # every figure as a share of the WHOLE frame's raw MSE: the background's part is err[bg].mean()·share
            part = lambda key: " ".join(f"{x:.4f}" for x in (row[key][0] / whole, row[key][1] * row["share_background"] / whole,  # noqa: E731
                                                             row[key][2] * (1 - row["share_background"]) / whole))
            print(f"frame {k:2d}: MSE / raw of the frame (all | background's part | hit pixels' part): temporal input {part('temporal_input')}, "
                  f"accumulate {part('temporal_accumulate')}; + guided input {part('temporal_guided_input')}, accumulate "
                  f"{part('temporal_guided_accumulate')}; background found {row['background_found']:.4f}, mean length "
                  f"{row['background_mean_length']:.1f}", flush=True)
        print(f"raw MSE of the last frame (all | background | hit): {row['raw']}; background share {row['share_background']:.4f}", flush=True)
        for tm in tms.values():
            tm.close()
        dn.close()
    ds.close()
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


CLIP_GAMMAS = (0.5, 1.0, 2.0, float("inf"))


def main_clip(args):
    """--clip: see the module docstring."""
    render.init(0)
    t = tracer.randomBouncing(args.width, seed=42) if args.config == 2 else tracer.randomBouncing(args.width, -50, 50, seed=42)
    t.samples_per_px, t.max_bounces = args.spp, 50
    t.set_gpu(render_seed=1, traversal=capi.TRAVERSAL_BVH, chunk_spp=0)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    p.tmin = 1e-3
    w, h = p.width, p.height
    n = w * h
    assert args.spp <= 16, "--clip wants an spp of at most 16: one automatic chunk"
    ds = render.DeviceScene(sd)
    move = (lambda k: orbited(cam, args.pan * k, w, h)) if args.motion == "orbit" else (lambda k: panned(cam, args.pan * k))
    res = {"mode": "clip", "config": args.config, "motion": args.motion, "size": f"{w}x{h}", "frames": args.frames,
           "px_per_frame": args.pan, "spp": args.spp, "ref_spp": args.ref_spp, "reps": args.reps}
    seq = []
    for k in range(args.frames if not args.cost_only else 2):
        c = move(k)
        q = capi.RenderParams.from_buffer_copy(p)
        q.seed, q.chunk_spp = 1000 + k, 0
        one = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        ds.render_into(c, q, one.data_ptr())
        ds.sync()
        g = ds.gbuffer(c, p)
        ds.query_sync()
        ref = None
        if not args.cost_only:
            q.samples_per_px, q.seed = args.ref_spp, 7
            ref = torch.empty_like(one)
            torch.cuda.synchronize()
            ds.render_into(c, q, ref.data_ptr())
            ds.sync()
        seq.append((c, one, g, ref))
        print(f"frame {k}: {args.spp} spp in one chunk, background {float((g.index < 0).float().mean()):.4f} of the pixels"
              + ("" if ref is None else f", reference {args.ref_spp} spp"), flush=True)
    var = torch.full((h, w, 3), 1e-3, dtype=torch.float32, device="cuda")  # (the plain step's cost does not depend on the variance's values)
    out, vout = torch.empty((h, w, 3), dtype=torch.float32, device="cuda"), torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    clipped = torch.zeros((h, w), dtype=torch.uint8, device="cuda")

    # ---- (a) cost: the moved step, OFF and VARIANCE alternating; and the moments step's first frame ------------------------------
    res["cost"] = {}
    clips = ("off", "variance")
    handles = {(kind, bg, clip): render.Temporal(w, h, moments=kind == "moments", background=bg)
               for kind in ("plain", "moments") for bg in ("input", "accumulate") for clip in clips}
    for (kind, bg, clip), tm in handles.items():
        tm.set_clip(clip, clipped=clipped if clip == "variance" else False)

    def steps(kind, tm, frames):
        tm.reset()
        for c, one, g, _ in frames:
            if kind == "plain":
                tm.step(one, var, g, c, args.spp, out=out, var_out=vout)
            else:
                tm.step_moments(one, g, c, args.spp, out=out, var_out=vout)

    ms = {k: [] for k in handles}
    first = []
    for r in range(args.warmup + args.reps):
        for (kind, bg, clip), tm in handles.items():
            steps(kind, tm, seq[:2])
            x = tm.timing()
            if r >= args.warmup:
                ms[(kind, bg, clip)].append(x)
        tm = handles[("moments", "input", "off")]
        steps("moments", tm, seq[:1])
        x = tm.timing()
        if r >= args.warmup:
            first.append(x)
    for kind, nbytes in (("plain", STEP_BYTES), ("moments", MOMENTS_STEP_BYTES)):
        for bg in ("input", "accumulate"):
            med = {clip: statistics.median(ms[(kind, bg, clip)]) for clip in clips}
            for clip in clips:
                per_pixel = nbytes + (1 if clip == "variance" else 0)  # (the variance handles here write the clipped bytes)
                cp = copy_ms(n * per_pixel // 2, args.reps, args.warmup)
                v = ms[(kind, bg, clip)]
                share = None
                if clip == "variance":
                    steps(kind, handles[(kind, bg, clip)], seq[:2])
                    torch.cuda.synchronize()
                    share = float(clipped.float().mean())
                res["cost"][f"{kind} {bg} {clip}"] = {"ms": med[clip], "min": min(v), "max": max(v), "bytes_per_pixel": per_pixel, "copy_ms": cp[0],
                                                      "copy_min": cp[1], "copy_max": cp[2], "ratio_to_copy": med[clip] / cp[0],
                                                      "ratio_to_off": med[clip] / med["off"], "clipped_share": share}
                print(f"{kind:7s} moved step, background {bg:10s}, clip {clip:8s}: {med[clip]:.4f} ms [{min(v):.4f}, {max(v):.4f}] = "
                      f"{med[clip] / cp[0]:.2f} x the copy of its {per_pixel} B per pixel ({cp[0]:.4f} ms [{cp[1]:.4f}, {cp[2]:.4f}]), "
                      f"{med[clip] / med['off']:.3f} x the off mode" + ("" if share is None else f"; {share:.4f} of the pixels clipped"), flush=True)
    cp = copy_ms(n * MOMENTS_STEP_BYTES // 2, args.reps, args.warmup)
    fm = statistics.median(first)
    res["cost"]["moments first frame"] = {"ms": fm, "min": min(first), "max": max(first), "copy_ms": cp[0], "ratio_to_copy": fm / cp[0]}
    print(f"moments FIRST frame (stages in every workgroup): {fm:.4f} ms [{min(first):.4f}, {max(first):.4f}] = {fm / cp[0]:.2f} x the copy of its "
          f"{MOMENTS_STEP_BYTES} B per pixel ({cp[0]:.4f} ms)", flush=True)
    for tm in handles.values():
        tm.close()

    # ---- (b) quality: moments handles on the one-chunk frames ---------------------------------------------------------------------
    if not args.cost_only:
        dn = render.Denoiser(w, h)
        den = torch.empty_like(out)
        res["rows"] = []
        names = ["off"] + [f"g{g_}" for g_ in CLIP_GAMMAS]
        tms = {}
        for bg in ("input", "accumulate"):
            tms[(bg, "off")] = render.Temporal(w, h, moments=True, background=bg)
            for g_ in CLIP_GAMMAS:
                tms[(bg, f"g{g_}")] = render.Temporal(w, h, moments=True, background=bg, clip="variance", clip_gamma=g_)
                tms[(bg, f"g{g_}")].set_clip("variance", g_, clipped=clipped)
        for k, (c, one, g, ref) in enumerate(seq):
            bgm = g.index < 0

            def mse2(a):
                err = ((a.double() - ref.double()) ** 2).mean(dim=2)
                return [float(err.mean()), float(err[bgm].mean()) if bool(bgm.any()) else 0.0, float(err[~bgm].mean())]

            row = {"frame": k, "raw": mse2(one), "share_background": float(bgm.float().mean())}
            for (bg, name), tm in tms.items():
                tm.step_moments(one, g, c, args.spp, out=out, var_out=vout)
                dn.run_guided(out, vout, g, out=den)
                torch.cuda.synchronize()
                row[f"temporal_{bg}_{name}"], row[f"temporal_guided_{bg}_{name}"] = mse2(out), mse2(den)
                if name != "off":
                    row[f"clipped_{bg}_{name}"] = float(clipped.float().mean())
            res["rows"].append(row)
            whole = row["raw"][0]  # every figure as a share of the WHOLE frame's raw MSE, as --background prints them
            sb = row["share_background"]
            part = lambda key: "/".join(f"{x:.4f}" for x in (row[key][0] / whole, row[key][1] * sb / whole, row[key][2] * (1 - sb) / whole))  # noqa: E731
            for bg in ("input", "accumulate"):
                print(f"frame {k:2d} {bg:10s}: MSE / raw of the frame (all/background's part/hit pixels' part): "
                      + "; ".join(f"{name} {part(f'temporal_{bg}_{name}')} +guided {part(f'temporal_guided_{bg}_{name}')}"
                                  + ("" if name == "off" else f" clipped {row[f'clipped_{bg}_{name}']:.4f}") for name in names), flush=True)
        print(f"raw MSE of the last frame (all | background | hit): {row['raw']}; background share {row['share_background']:.4f}", flush=True)
        for tm in tms.values():
            tm.close()
        dn.close()
    ds.close()
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--pan", type=float, default=3.0, help="pixels per frame")
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--chunk-spp", type=int, default=2)
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--json", default=None, help="also write the figures to this file")
    ap.add_argument("--moments", action="store_true", help="measure the moments mode (DESIGN.md §4.16) beside the plain step")
    ap.add_argument("--settle", type=int, default=6, help="--moments: static frames behind a 'settled' history (W2 = 1 / settle)")
    ap.add_argument("--feedback", action="store_true", help="measure the feedback of the filtered colour (DESIGN.md §4.17) beside the moments step")
    ap.add_argument("--counts", action="store_true", help="measure the counts step (DESIGN.md §4.23) beside the scalar steps")
    ap.add_argument("--cubic", action="store_true", help="measure the cubic resampling mode (DESIGN.md §4.26) beside the bilinear one")
    ap.add_argument("--background", action="store_true", help="measure the background mode (DESIGN.md §4.27) beside the input mode")
    ap.add_argument("--clip", action="store_true", help="measure the clip mode (DESIGN.md §4.28) beside the off mode")
    ap.add_argument("--cost-only", action="store_true", help="--cubic, --background, --clip: the cost part alone (two frames, no references)")
    ap.add_argument("--config", type=int, default=3, choices=(2, 3), help="--cubic: BASELINE config 2 (grid [-11, 11)) or 3 (grid [-50, 50))")
    ap.add_argument("--motion", default="pan", choices=("pan", "orbit"),
                    help="--cubic: pan (px_origin moved along px_du by --pan pixels per frame) or orbit (look_from turned about the focus point by --pan "
                         "pixel widths per frame)")
    ap.add_argument("--lib-label", default=None, help="--cubic: what to call --lib's build in the output")
    ap.add_argument("--lib", default=None, help="--cubic: load this build of librayz_hip.so (an older one: its bilinear step alone is timed)")
    args = ap.parse_args()
    if args.clip:
        return main_clip(args)
    if args.background:
        return main_background(args)
    if args.cubic:
        return main_cubic(args)
    if args.counts:
        return main_counts(args)
    if args.feedback:
        return main_feedback(args)
    if args.moments:
        return main_moments(args)
    render.init(0)
    t = tracer.randomBouncing(args.width, -50, 50, seed=42)  # config 3
    t.samples_per_px, t.max_bounces = args.spp, 50
    t.set_gpu(render_seed=1, traversal=capi.TRAVERSAL_BVH, chunk_spp=args.chunk_spp)
    sd, cam, p = t.scene_desc(), t.camera_desc(), t.params()
    p.tmin = 1e-3
    w, h = p.width, p.height
    n = w * h
    ds = render.DeviceScene(sd)
    res = {"size": f"{w}x{h}", "frames": args.frames, "pan_px": args.pan, "spp": args.spp, "chunk_spp": args.chunk_spp, "ref_spp": args.ref_spp,
           "reps": args.reps, "step_bytes_per_pixel": STEP_BYTES}

    # ---- the sequence: frame, variance, G-buffer and reference per camera ----------------------------------------------------
    seq = []
    for k in range(args.frames):
        c = panned(cam, args.pan * k)
        q = capi.RenderParams.from_buffer_copy(p)
        q.seed = 1000 + k
        pr = ds.progressive(c, q, track_noise=True)
        frame = torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        while not pr.done:
            pr.step(0, frame.data_ptr())
        assert pr.chunks_done >= 2, "a frame needs at least 2 chunks for a variance estimate"
        var = pr.noise_rgb()
        trace_ms = pr.stats().kernel_ms
        pr.close()
        g = ds.gbuffer(c, p)
        ds.query_sync()
        q.samples_per_px, q.chunk_spp, q.seed = args.ref_spp, 0, 7
        ref = torch.empty_like(frame)
        torch.cuda.synchronize()
        ds.render_into(c, q, ref.data_ptr())
        ds.sync()
        seq.append((c, frame, var, g, ref, trace_ms))
        print(f"frame {k}: {args.spp} spp in chunks of {args.chunk_spp} ({trace_ms:.2f} ms of trace kernels), reference {args.ref_spp} spp", flush=True)
    res["frame_trace_ms"] = statistics.median(s[5] for s in seq)
    mse = lambda a, ref: float(((a.double() - ref.double()) ** 2).mean())  # noqa: E731

    # ---- (a) cost -------------------------------------------------------------------------------------------------------------
    cp = copy_ms(n * STEP_BYTES // 2, args.reps, args.warmup)
    print(f"copy moving a step's compulsory bytes ({n * STEP_BYTES / 1e6:.1f} MB read + written): {cp[0]:.4f} ms [{cp[1]:.4f}, {cp[2]:.4f}] "
          f"({n * STEP_BYTES / cp[0] / 1e9:.2f} TB/s)", flush=True)
    res["copy_ms"], res["copy_min"], res["copy_max"] = cp
    tm = render.Temporal(w, h)
    out, vout = torch.empty((h, w, 3), dtype=torch.float32, device="cuda"), torch.empty((h, w, 3), dtype=torch.float32, device="cuda")
    length = torch.empty((h, w), dtype=torch.float32, device="cuda")
    res["cost"] = {}
    for what in ("first", "static", "panned"):
        ms = []
        for r in range(args.warmup + args.reps):
            tm.reset()
            if what == "first":
                tm.step(seq[0][1], seq[0][2], seq[0][3], seq[0][0], args.spp, out=out, var_out=vout, length=length)
            else:
                tm.step(seq[0][1], seq[0][2], seq[0][3], seq[0][0], args.spp, out=out, var_out=vout, length=length)
                s = seq[0] if what == "static" else seq[1]
                tm.step(s[1], s[2], s[3], s[0], args.spp, out=out, var_out=vout, length=length)
            x = tm.timing()
            if r >= args.warmup:
                ms.append(x)
        med = statistics.median(ms)
        print(f"step kernel, {what:6s}: {med:.4f} ms [{min(ms):.4f}, {max(ms):.4f}] = {med / cp[0]:.2f} x the copy of its compulsory bytes "
              f"({n * STEP_BYTES / med / 1e9:.2f} TB/s of them); {med / res['frame_trace_ms']:.4f} x the {args.spp}-spp frame's trace kernels", flush=True)
        res["cost"][what] = {"ms": med, "min": min(ms), "max": max(ms), "ratio_to_copy": med / cp[0]}

    # ---- (b), (c) at the defaults; (d) the sweep ---------------------------------------------------------------------------------
    dn = render.Denoiser(w, h)
    den = torch.empty_like(out)

    def run(guided_too, **prm):
        tm.reset()
        rows = []
        for k, (c, frame, var, g, ref, _) in enumerate(seq):
            tm.step(frame, var, g, c, args.spp, out=out, var_out=vout, length=length, **prm)
            torch.cuda.synchronize()
            hit = g.index >= 0
            row = {"frame": k, "mse_raw": mse(frame, ref), "mse_temporal": mse(out, ref),
                   "found": float((length[hit] > args.spp).float().mean()) if bool(hit.any()) else 0.0}
            if guided_too:
                dn.run_guided(out, vout, g, out=den)
                torch.cuda.synchronize()
                row["mse_temporal_guided"] = mse(den, ref)
            rows.append(row)
        return rows

    rows = run(True)
    for row, (c, frame, var, g, ref, _) in zip(rows, seq):
        dn.run_guided(frame, var, g, out=den)
        torch.cuda.synchronize()
        row["mse_guided"] = mse(den, ref)
        r = row["mse_raw"]
        print(f"frame {row['frame']:2d}: MSE raw {r:.4e}; guided alone x{row['mse_guided'] / r:.4f}; temporal alone x{row['mse_temporal'] / r:.4f}; "
              f"temporal + guided x{row['mse_temporal_guided'] / r:.4f}; {row['found']:.4f} of the hit pixels found history", flush=True)
    res["defaults"] = {"params": capi.TEMPORAL_DEFAULTS, "rows": rows}
    res["sweep"] = []
    for am in (0.0, 0.05, 0.1, 0.2):
        for md in (0.01, 0.05, 0.2):
            rr = run(True, alpha_min=am, max_rel_dist=md)[1:]
            mean = lambda key: statistics.mean(x[key] / x["mse_raw"] for x in rr)  # noqa: E731
            row = {"alpha_min": am, "max_rel_dist": md, "temporal": mean("mse_temporal"), "temporal_guided": mean("mse_temporal_guided"),
                   "found": statistics.mean(x["found"] for x in rr), "last_temporal": rr[-1]["mse_temporal"] / rr[-1]["mse_raw"],
                   "last_temporal_guided": rr[-1]["mse_temporal_guided"] / rr[-1]["mse_raw"]}
            res["sweep"].append(row)
            print(f"  alpha_min {am:g} max_rel_dist {md:g}: mean over frames 1.. of MSE / raw: temporal {row['temporal']:.4f}, temporal + guided "
                  f"{row['temporal_guided']:.4f} (last frame {row['last_temporal']:.4f}, {row['last_temporal_guided']:.4f}); found {row['found']:.4f}",
                  flush=True)
    tm.close()
    dn.close()
    ds.close()
    print(json.dumps(res), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
