#!/usr/bin/env python3
"""Primary lists forced OFF and ON on the benchmark's scenes at 1920x1080, one JSON line per render to stdout.

  python tools/primary_lists_table.py forms     config 3 at 16 spp and config 2 at 64 spp under XZ, XY and ONE_RADIUS, f32 and f64
  python tools/primary_lists_table.py gates     both sides of AUTO's gates: 10,003 spheres at 4 .. 64 spp, 100 .. 4,097 spheres at 256 spp

One DeviceScene per (grid, spp); per precision and scan form the second of two renders with the lists OFF and ON: kernel ms (the
library's events, the builder inside them), segments, the frame's hash.  Asserts that the frames and segments of each (scene,
precision) group are equal.  Run from the repository's root; wrote profiles/r15/primary_lists/forms_equal.txt and gates.jsonl."""
import hashlib, json, sys
import torch
sys.path.insert(0, ".")
from rayz_amd import capi, render, tracer

render.init(0)
FORMS = {"auto": capi.SCAN_FORM_AUTO, "xz": capi.SCAN_FORM_XZ, "xy": capi.SCAN_FORM_XY, "one": capi.SCAN_FORM_ONE_RADIUS}
rows = []
def run(grid, spp, precs, forms, modes=("off", "on")):
    t = tracer.randomBouncing(1920, -grid, grid, seed=42)
    t.samples_per_px, t.max_bounces = spp, 50
    t.set_gpu(render_seed=1, traversal=capi.TRAVERSAL_LINEAR)
    scene, cam = t.scene_desc(), t.camera_desc()
    ds = render.DeviceScene(scene)
    for prec in precs:
        t.set_gpu(precision=prec)
        p = t.params()
        out = torch.empty((p.height, p.width, 3), dtype=torch.float64 if prec == capi.PRECISION_F64 else torch.float32, device="cuda")
        group = []
        for form in forms:
            ds.scan_form = FORMS[form]
            for mode in modes:
                ds.set_primary_lists({"off": capi.PRIMARY_LISTS_OFF, "on": capi.PRIMARY_LISTS_ON, "auto": capi.PRIMARY_LISTS_AUTO}[mode])
                ms = []
                for _ in range(2):
                    torch.cuda.synchronize()
                    ds.render_into(cam, p, out.data_ptr())
                    st = ds.sync()
                    ms.append(st.kernel_ms)
                h = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]
                row = dict(grid=grid, spheres=scene.n_spheres, spp=spp, precision=int(prec), form=form, form_used=ds.scan_form, lists=mode,
                           uses=ds.uses_primary_lists(spp), kernel_ms=round(ms[1], 3), first_ms=round(ms[0], 3), segments=st.segments, sha=h,
                           finite=bool(torch.isfinite(out).all()))
                group.append(row)
                print(json.dumps(row), flush=True)
        assert len({(r["sha"], r["segments"]) for r in group}) == 1, "frames or segments differ"
    ds.close()

which = sys.argv[1]
F32, F64 = capi.PRECISION_F32, capi.PRECISION_F64
if which == "forms":  # the forced-form table
    run(50, 16, (F32, F64), ("xz", "xy", "one"))
    run(11, 64, (F32, F64), ("xz", "xy", "one"))
elif which == "gates":  # both sides of AUTO's gates, the scan form AUTO's
    for spp in (4, 8, 16, 32, 64):
        run(50, spp, (F32,), ("auto",))
    for grid in (5, 8, 11, 16, 22, 32):
        run(grid, 256, (F32,), ("auto",))
    run(11, 32, (F32,), ("auto",))
    run(16, 32, (F32,), ("auto",))
print("ok")
