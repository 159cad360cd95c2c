#!/usr/bin/env python3
"""The cell lists' tables (profiles/r18/cell_lists/): kernel ms of randomBouncing frames at 1920x1080 on one
DeviceScene, cells OFF / ON / AUTO.  One JSON line per run, printed and appended to OUT.

  python tools/cell_lists_table.py TREE OUT profile   the default frame, OFF and ON at kMaxCells 4 / 6 / 9 / 12 (a -DRAYZ_FLAT_PROFILE
                                                      -DRAYZ_CELLS_TUNE build of TREE: the phases go to stderr)
  python tools/cell_lists_table.py TREE OUT sweep     kListLanes x kMaxCells on the default frame (a -DRAYZ_CELLS_TUNE build)
  python tools/cell_lists_table.py TREE OUT walk      the walk (profiles/r21/cell_walk/): kWalkColumns x the lane rule at 16 lanes, then
                                                      kListLanes 8 / 16 / 24 at the best two (a -DRAYZ_CELLS_TUNE build)
  python tools/cell_lists_table.py TREE OUT walk_at COLUMNS:LANES ..  single points of that sweep, two launches each
  python tools/cell_lists_table.py TREE OUT walk_grid GRID SPP COLUMNS:LANES ..  the same points on another grid, OFF first
  python tools/cell_lists_table.py TREE OUT walk_profile  the default frame, ON without the walk and with it (a -DRAYZ_FLAT_PROFILE
                                                      -DRAYZ_CELLS_TUNE build: the phases go to stderr; with
                                                      -DRAYZ_FLAT_PROFILE_WALK as well, the histogram of the box-unlistable
                                                      segments by the columns of their walk and the walk's cells per bin; arguments:
                                                      the caps to run, as COLUMNS or COLUMNS:LANES)
  python tools/cell_lists_table.py TREE OUT gates [GRID ..]  OFF against ON at grids 5 .. 50 (or those named), 256 spp (the product build)
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
    return min(ms)


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
elif what == "walk":  # the tune build: the walk's column cap x the lane rule, then the lanes at the best two
    t = scene(50, 1024)
    ds = render.DeviceScene(t.scene_desc())
    run(ds, t, "headline off", OFF)
    ms = {}
    for wc in (0, 8, 12, 16, 24, 32, 48):
        for one in (0, 1):
            if wc or not one:  # (without a walk there is one class anyway)
                ms[(wc, one)] = run(ds, t, "headline on", ON, RAYZ_CELLS_WALK_COLUMNS=wc, RAYZ_CELLS_ONE_CLASS=one, RAYZ_CELLS_LIST_LANES=16)
    for wc, one in sorted(ms, key=ms.get)[:2]:
        for ll in (8, 24):
            run(ds, t, "headline on", ON, RAYZ_CELLS_WALK_COLUMNS=wc, RAYZ_CELLS_ONE_CLASS=one, RAYZ_CELLS_LIST_LANES=ll)
elif what == "walk_at":  # the tune build: the configurations named as COLUMNS:LANES
    t = scene(50, 1024)
    ds = render.DeviceScene(t.scene_desc())
    for a in sys.argv[4:]:
        wc, ll = map(int, a.split(":"))
        run(ds, t, "headline on", ON, reps=2, RAYZ_CELLS_WALK_COLUMNS=wc, RAYZ_CELLS_ONE_CLASS=0, RAYZ_CELLS_LIST_LANES=ll)
elif what == "walk_grid":  # the tune build: another grid (GRID SPP) at the configurations named, OFF first
    t = scene(int(sys.argv[4]), int(sys.argv[5]))
    ds = render.DeviceScene(t.scene_desc())
    run(ds, t, f"grid {sys.argv[4]} off", OFF, reps=2)
    for a in sys.argv[6:]:
        wc, ll = map(int, a.split(":"))
        run(ds, t, f"grid {sys.argv[4]} on", ON, reps=2, RAYZ_CELLS_WALK_COLUMNS=wc, RAYZ_CELLS_ONE_CLASS=0, RAYZ_CELLS_LIST_LANES=ll)
elif what == "walk_profile":  # the profile build: phases to stderr
    t = scene(50, 1024)
    ds = render.DeviceScene(t.scene_desc())
    run(ds, t, "headline on, no walk", ON, RAYZ_CELLS_WALK_COLUMNS=0, RAYZ_CELLS_LIST_LANES=16)
    for wc in sys.argv[4:] or ("12",):
        wc, ll = (wc.split(":") + ["16"])[:2]
        run(ds, t, f"headline on, walk {wc}", ON, RAYZ_CELLS_WALK_COLUMNS=int(wc), RAYZ_CELLS_LIST_LANES=int(ll))
elif what == "gates":  # the product build: OFF against ON at 256 spp
    for g in map(int, sys.argv[4:] or (5, 8, 11, 16, 22, 32, 50)):
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
