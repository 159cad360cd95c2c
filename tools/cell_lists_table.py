#!/usr/bin/env python3
"""The cell lists' tables (profiles/r18/cell_lists/): kernel ms of randomBouncing frames at 1920x1080 on one
DeviceScene, cells OFF / ON / AUTO.  One JSON line per run, printed and appended to OUT.

  python tools/cell_lists_table.py TREE OUT profile   the default frame, OFF and ON at kMaxCells 4 / 6 / 9 / 12 (a -DRAYZ_FLAT_PROFILE
                                                      -DRAYZ_CELLS_TUNE build of TREE: the phases go to stderr)
  python tools/cell_lists_table.py TREE OUT sweep     kListLanes x kMaxCells on the default frame (a -DRAYZ_CELLS_TUNE build)
  python tools/cell_lists_table.py TREE OUT gates     OFF against ON at grids 5 .. 50, 256 spp (the product build)
  python tools/cell_lists_table.py TREE OUT rows      the other benchmark rows under AUTO (run once per build, a tree of the parent
                                                      commit included: it has no cells and ignores the mode)

TREE: the source tree whose built library is measured ("." for this one)."""
import hashlib, json, os, sys
tree, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
sys.path.insert(0, tree)
import torch
from rayz_amd import capi, render, tracer

assert os.path.dirname(os.path.dirname(os.path.abspath(capi.__file__))) == tree, capi.__file__
render.init(0)
out_f = open(out_path, "a")


def scene(grid, spp, prec=capi.PRECISION_F32, width=1920):
    t = tracer.randomBouncing(width, -grid, grid, seed=42)
    t.samples_per_px, t.max_bounces = spp, 50
    t.set_gpu(render_seed=1, precision=prec, traversal=capi.TRAVERSAL_LINEAR)
    return t


def run(ds, t, tag, cells, reps=1, **env):
    for k, v in env.items():
        os.environ[k] = str(v)
    cam, p = t.camera_desc(), t.params()
    dt = torch.float64 if p.precision == capi.PRECISION_F64 else torch.float32
    out = torch.zeros((render.shard_rows(p), p.width, 3), dtype=dt, device="cuda")
    torch.cuda.synchronize()
    if hasattr(ds, "set_cell_lists"):
        ds.set_cell_lists(cells)
    ms = []
    for _ in range(reps):
        ds.render_into(cam, p, out.data_ptr())
        st = ds.sync()
        ms.append(round(st.kernel_ms, 2))
    sha = hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest()[:16]
    rec = dict(tag=tag, cells=cells, uses=ds.uses_cell_lists() if hasattr(ds, "uses_cell_lists") else None, kernel_ms=ms, segments=int(st.segments), sha=sha, **env)
    print(json.dumps(rec), flush=True)
    out_f.write(json.dumps(rec) + "\n")
    out_f.flush()


what = sys.argv[3]
OFF, ON, AUTO = 1, 2, 0  # capi.CELL_LISTS_* (the parent tree has none)
if what == "profile":  # the profile build: phases to stderr
    t = scene(50, 1024)
    ds = render.DeviceScene(t.scene_desc())
    run(ds, t, "headline off", OFF)
    for mc in (4, 6, 9, 12):
        run(ds, t, f"headline on max_cells {mc}", ON, RAYZ_CELLS_MAX_CELLS=mc, RAYZ_CELLS_LIST_LANES=16)
elif what == "sweep":  # the tune build
    t = scene(50, 1024)
    ds = render.DeviceScene(t.scene_desc())
    run(ds, t, "headline off", OFF, reps=2)
    for mc in (9, 12):
        for ll in (4, 8, 16, 24, 32):
            run(ds, t, f"headline on", ON, RAYZ_CELLS_MAX_CELLS=mc, RAYZ_CELLS_LIST_LANES=ll)
    for mc in (4, 6):
        run(ds, t, f"headline on", ON, RAYZ_CELLS_MAX_CELLS=mc, RAYZ_CELLS_LIST_LANES=16)
elif what == "gates":  # the product build: OFF against ON at 256 spp
    for g in (5, 8, 11, 16, 22, 32, 50):
        t = scene(g, 256)
        ds = render.DeviceScene(t.scene_desc())
        n = t.info().n_spheres
        run(ds, t, f"grid {g} ({n} spheres) off", OFF, reps=3)
        run(ds, t, f"grid {g} ({n} spheres) on", ON, reps=3)
        run(ds, t, f"grid {g} ({n} spheres) off", OFF, reps=2)
        run(ds, t, f"grid {g} ({n} spheres) on", ON, reps=2)
        ds.close()
elif what == "rows":  # nobody else pays: the product build under AUTO (run once per tree)
    rows = [("config 2", 11, 1024, capi.PRECISION_F32), ("grid 5", 5, 1024, capi.PRECISION_F32), ("config 3 16 spp", 50, 16, capi.PRECISION_F32),
            ("config 3 64 spp", 50, 64, capi.PRECISION_F32), ("config 3 128 spp", 50, 128, capi.PRECISION_F32),
            ("f64 16 spp", 50, 16, capi.PRECISION_F64), ("grid 15 256 spp", 15, 256, capi.PRECISION_F32), ("grid 16 256 spp", 16, 256, capi.PRECISION_F32)]
    for name, g, spp, prec in rows:
        t = scene(g, spp, prec)
        ds = render.DeviceScene(t.scene_desc())
        run(ds, t, name, AUTO, reps=3)
        ds.close()
