"""The walk, the second tier of the cells' query: `cells_stretch`, `cells_walk` and `walk_column` of
rayz_amd/csrc/slab_cells.hpp, compiled into a stand-alone host program (tests/slab_walk_mirror.cpp) beside the box of `cells_query`.

Per pool of test_slab_cells_cpu.py: 20,000 of its rays, 3,400 CONSTRUCTED ones — an origin inside the slab or up to 2 above it, aimed at
a member's position at the ray's time (offset 0.9·|r|) 3 to cap − 4 cells away, kept if the whole stretch inside the slab (it goes on
behind the target until it leaves the slab) crosses at most cap − 1 columns by this file's own arithmetic — and 600 CAP rays: level
stretches nearly along x or z, cap − 2 to cap + 0.5 cells long over two rows or more, that enter the slab from above.  The cap is the
product's kWalkColumns where the grid is at least twice as wide (the headline pool) and 8 elsewhere (the lattices are 10 to 22 cells wide): the mirror is a
-DRAYZ_CELLS_TUNE build and takes it as an argument.  The mirror decides every (ray, member) pair with the exact f64 quadratic.

Mutations of the header, each run once against this file and each failing it (not committed; figures of the pools at a cap of 8):
  * the column dilation dropped (pm = 0 in walk_column): `misses` fails in five pools (config2 1, negative_radii 1, slab_at_zero 2,
    slab_at_3e4 1, borders_and_edge 70); the headline pool and cap_and_cap_plus_one do not notice — the band and the neighbouring
    columns' dilated ranges cover most of what a column's own edge loses;
  * the minor dilation dropped (pn = 0, and the band's half-width without it): `misses` fails in every pool (config2 33,
    negative_radii 25, slab_at_zero 73, slab_at_3e4 46, cap_and_cap_plus_one 3, borders_and_edge 877) and with it `target_ok`; the
    hand cases fail on their cell counts (8 for 16);
  * the sub-stretch not clipped to [t0, t1] and the ranges not to the box: no miss, `outside_box` fails in every pool (config2 1,877
    cells, slab_at_zero 975) and in the hand cases;
  * the last column left out (k1 - 1 in cells_walk; the mutant must guard k1 = 0, or its loop runs 2^32 times): `misses` fails in
    every pool (slab_at_zero 578, slab_at_3e4 495, cap_and_cap_plus_one 397, borders_and_edge 972), the hand cases on their columns;
  * the overflow pre-walk skipped: cap_and_cap_plus_one fails `misses` (25) and `a walk through the overflowed cell is not listable`,
    borders_and_edge fails `misses` (30);
  * the major axis always x: no miss (a walk along the minor axis is still a superset, its columns only hold more cells), but
    `over_three` fails in every pool (config2 1,352 rays), the hand cases fail on the axis and the strip scene has no ray over the cap;
  * the band dropped (the issue's range alone): no miss; `over_three` fails in slab_at_3e4 (39 rays: eps is 0.12 there, and a
    column dilated by 0.32 on each side can reach a fourth cell), and every pool names 4 to 8 % more cells.
kRel and kEvalRel are NOT reached, as in test_slab_cells_cpu.py: with both 0 this file passes.  They rest on §4.22's proof."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from test_plane_runs import _write
from test_slab_cells_cpu import N_RAYS, POOLS, TMIN, _lattice, members_of, pool, rays

HERE = os.path.dirname(os.path.abspath(__file__))
N_AIMED, N_CAP = 3_400, 600
NONE, BOX, WALK, SCAN = 0, 1, 2, 3


@pytest.fixture(scope="module")
def wmirror(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("slab_walk") / "slab_walk_mirror")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-DRAYZ_CELLS_TUNE", "-o", exe, os.path.join(HERE, "slab_walk_mirror.cpp")],
                   check=True, capture_output=True, timeout=300)
    return exe


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def grid_of(s):
    """The grid build_cells makes of the pool `s` (test_slab_cells_cpu.py holds the builder to this)."""
    cand = (s[:, 3] == 0) & (s[:, 5] == 0)
    side = np.sqrt((s[cand, 0].max() - s[cand, 0].min()) * (s[cand, 2].max() - s[cand, 2].min()) / cand.sum())
    cell = 2.0 ** np.floor(np.log2(side) + 0.5)
    m = s[members_of(s, cell)]
    ra = np.abs(m[:, 6])
    x0, z0 = np.floor(m[:, 0].min() / cell) * cell, np.floor(m[:, 2].min() / cell) * cell
    return dict(cell=cell, x0=x0, z0=z0, nx=int(np.floor((m[:, 0].max() - x0) / cell)) + 1, nz=int(np.floor((m[:, 2].max() - z0) / cell)) + 1,
                ylo=(np.minimum(m[:, 1], m[:, 1] + m[:, 4]) - ra).min(), yhi=(np.maximum(m[:, 1], m[:, 1] + m[:, 4]) + ra).max(), rmax=ra.max(),
                extent=(np.abs(m[:, :3]).sum(axis=1) + np.abs(m[:, 4]) + ra).max())


def columns(o, d, g):
    """Per ray: the index ranges (x and z, before the clip) of its stretch inside the slab, dilated by rmax, by this file's arithmetic."""
    eps = 1e-3 + 2e-6 * (np.abs(o).sum(axis=1) + g["extent"])  # (above eps of slab_cells.hpp: 0.12 for a slab at 3e4, in y too)
    with np.errstate(divide="ignore", invalid="ignore"):
        ta, tb = (g["ylo"] - eps - o[:, 1]) / d[:, 1], (g["yhi"] + eps - o[:, 1]) / d[:, 1]
    t0, t1 = np.maximum(np.minimum(ta, tb), 0.0), np.maximum(ta, tb)
    out = []
    for ax, org in ((0, g["x0"]), (2, g["z0"])):
        a, b = o[:, ax] + t0 * d[:, ax], o[:, ax] + t1 * d[:, ax]
        p = g["rmax"] + eps
        out.append((np.floor((np.minimum(a, b) - p - org) / g["cell"]), np.floor((np.maximum(a, b) + p - org) / g["cell"])))
    return out


def constructed(rng, s, g, cap, n, targets=None):
    """(n, 8) aimed rays: {o, d, time, target row}."""
    mem = np.flatnonzero(members_of(s, g["cell"]))
    got = []
    while sum(map(len, got)) < n:
        k = 8 * n
        row = rng.choice(mem if targets is None else targets, k)
        time = rng.uniform(0.0, 1.0, k)
        centre = s[row, :3] + s[row, 3:6] * time[:, None]
        dist = rng.uniform(3.0, cap - 4.0, k) * g["cell"]
        az = rng.uniform(0.0, 2.0 * np.pi, k)
        az[::5] = rng.choice([0.0, 0.5, 1.0, 1.5], len(az[::5])) * np.pi + rng.normal(0.0, 0.02, len(az[::5]))  # near an axis: level columns
        o = np.column_stack([centre[:, 0] + dist * np.cos(az), rng.uniform(g["ylo"], g["yhi"] + 2.0, k), centre[:, 2] + dist * np.sin(az)])
        u = rng.normal(size=(k, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        d = centre + 0.9 * np.abs(s[row, 6:7]) * rng.uniform(0.0, 1.0, (k, 1)) * u - o
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        d *= rng.choice([0.05, 1.0, 10.0], (k, 1))
        (i0, i1), (j0, j1) = columns(o, d, g)
        keep = (d[:, 1] != 0) & (np.maximum(i1 - i0, j1 - j0) + 1 <= cap - 1)
        got.append(np.column_stack([o, d, time, row])[keep])
    return np.vstack(got)[:n]


def cap_rays(rng, g, cap, n):
    """(n, 8): stretches nearly along x or z that enter the slab from just above it and are cap − 2 to cap + 0.5 cells long."""
    cell, h = g["cell"], g["yhi"] - g["ylo"]
    length = rng.uniform(cap - 2.0, cap + 0.5, n) * cell - 2.0 * g["rmax"]
    along_x = rng.uniform(size=n) < 0.5
    size = np.where(along_x, g["nx"], g["nz"]) * cell
    org = np.where(along_x, g["x0"], g["z0"])
    start = org + 0.3 * cell + rng.uniform(size=n) * np.maximum(size - length - 0.6 * cell, 0.0)
    sign = rng.choice([-1.0, 1.0], n)
    start = np.where(sign > 0, start, start + length)
    other = np.where(along_x, g["z0"] + rng.uniform(3.0, g["nz"] - 3.0, n) * cell, g["x0"] + rng.uniform(3.0, g["nx"] - 3.0, n) * cell)
    lift = rng.uniform(0.0, 0.05, n) * h  # above the slab: the stretch starts at its top
    dm = sign * length
    dn = rng.choice([-1.0, 1.0], n) * rng.uniform(0.1, 0.2, n) * length  # two rows at least: no box of 12 cells holds the stretch
    o = np.column_stack([np.where(along_x, start - dm * lift / h, other), g["yhi"] + lift, np.where(along_x, other, start - dm * lift / h)])
    d = np.column_stack([np.where(along_x, dm, dn), np.full(n, -h), np.where(along_x, dn, dm)])
    d *= rng.choice([0.05, 1.0, 10.0], (n, 1)) / np.linalg.norm(d, axis=1, keepdims=True)
    return np.column_stack([o, d, rng.uniform(0.0, 1.0, n), np.full(n, -1.0)])


def cap_of(wmirror, g):
    w = run(wmirror, "consts")["walk_columns"]
    return w if min(g["nx"], g["nz"]) >= 2 * w else 8


@pytest.mark.parametrize("name", POOLS)
def test_box_or_walk_names_every_member_a_listable_ray_hits(wmirror, tmp_path, name):
    s = pool(name)
    g = grid_of(s)
    cap = cap_of(wmirror, g)
    assert cap == (12 if name == "headline" else 8)
    rng = np.random.default_rng(11)
    extra = None
    if name == "cap_and_cap_plus_one":  # a fifth of the aimed rays at the overflowed cell (4, 3)'s centres: the pool's last kCellCap rows
        extra = constructed(rng, s, g, cap, 200, targets=np.arange(len(s) - 3, len(s)))
    own = rays(rng, s, dict(cell=g["cell"], ylo=g["ylo"], yhi=g["yhi"]), N_RAYS)
    aimed = constructed(rng, s, g, cap, N_AIMED)
    if extra is not None:
        aimed[:len(extra)] = extra
    capped = cap_rays(rng, g, cap, N_CAP)
    everything = np.vstack([np.column_stack([own, np.full(len(own), -1.0)]), aimed, capped])
    got = run(wmirror, "check", _write(tmp_path, "s.bin", s), _write(tmp_path, "r.bin", everything), TMIN, cap)
    cls, cols, ncells, ok = (np.array(got[k]) for k in ("cls", "cols", "ncells", "target_ok"))
    print(name, "cap", cap, {k: v for k, v in got.items() if not isinstance(v, list)}, "classes", np.bincount(cls, minlength=4).tolist(),
          "aimed classes", np.bincount(cls[N_RAYS:N_RAYS + N_AIMED], minlength=4).tolist())
    assert got["rays"] == N_RAYS + N_AIMED + N_CAP and (got["nx"], got["nz"], got["cell"]) == (g["nx"], g["nz"], g["cell"])
    assert got["parent_differs"] == 0  # cells_query answers as its parent text does
    assert got["misses"] == 0, got["first_miss"]
    assert got["twice"] == 0 and got["outside_box"] == 0
    assert 2 * g["rmax"] <= g["cell"] and got["over_three"] == 0
    assert (cls == WALK).sum() >= 1_000 and got["listed_hits"] >= 2_000
    a = slice(N_RAYS, N_RAYS + N_AIMED)
    (i0, i1), (j0, j1) = columns(aimed[:, :3], aimed[:, 3:6], g)
    inside = (i0 >= 0) & (i1 < g["nx"]) & (j0 >= 0) & (j1 < g["nz"])
    assert inside.sum() >= 500
    if not got["any_overflowed"]:
        assert not (cls[a][inside] == SCAN).any()  # by box or walk, none by the scan
    assert not (cls[a] == NONE).any()
    answered = (cls[a] == BOX) | (cls[a] == WALK)
    assert answered.sum() >= 2_000 and (ok[a][answered] == 1).all()  # every constructed ray's target is among its entries
    if extra is not None:  # a walk through the overflowed cell is not listable
        assert (cls[a][:len(extra)] == SCAN).all()
    c = slice(N_RAYS + N_AIMED, None)
    assert (cols[c] == cap).sum() >= 100 and (cols[c] == cap + 1).sum() >= 100 and (cols > cap).sum() >= 100
    assert (cls[cols > cap] == SCAN).all()
    if not got["any_overflowed"]:
        assert (cls[c][cols[c] == cap] == WALK).all()
    assert (ncells[cls == WALK] <= 3 * cols[cls == WALK]).all()


def test_hand_cases(wmirror, tmp_path):
    """A 12 x 12 lattice (cells of 1 from the origin, slab 0 .. 0.9 at most, rmax 0.2), cap 8."""
    s = _lattice(np.random.default_rng(1), 12)
    g = grid_of(s)
    assert (g["cell"], g["x0"], g["z0"], g["nx"], g["nz"]) == (1.0, 0.0, 0.0, 12, 12)
    h = g["yhi"]
    enter = 1.0 + 10.0 / (h + 1.0)  # where case 7 reaches the slab's top
    R = [
        [2.0, h, 5.0, 6.0, -h, 0.0],       # 0 axis-parallel, along x over the border of two rows: 8 columns of two cells
        [5.0, h, 9.0, 0.0, -h, -6.0],      # 1 .. along z
        [2.0, h, 2.0, 5.0, -h, 5.0],       # 2 exactly 45 degrees: the index ranges tie, z is major
        [2.0, h, 2.0, 5.0, -h, 4.0],       # 3 a little flatter in z: x is major
        [4.5, h, 5.0, 14.0, -h, 0.0],      # 4 leaves the grid mid-way: the columns end at the grid's last
        [-3.0, h, 5.0, 10.0, -h, 0.0],     # 5 starts outside it: the columns start at the grid's first
        [-9.0, h, 5.0, 7.0, -h, 0.0],      # 6 wholly beside it: no cells
        [1.0, h + 1.0, 4.0, 10.0, -(h + 1.0), 2.0],  # 7 starts above the slab: the stretch begins where it enters (three rows)
        [5.5, h + 1.0, 5.5, 0.0, -1.0, 0.0],         # 8 d.x = d.z = 0: a box
        [2.0, h, 5.0, 9.0, -h, 0.0],       # 9 eleven columns: over the cap
    ]
    r = np.column_stack([np.array(R), np.full(len(R), 0.5), np.full(len(R), -1.0)])
    got = run(wmirror, "check", _write(tmp_path, "s.bin", s), _write(tmp_path, "r.bin", r), TMIN, 8)
    cls, cols, ncells, xmajor = got["cls"], got["cols"], got["ncells"], got["xmajor"]
    print(cls, cols, ncells, xmajor)
    assert got["misses"] == 0 and got["twice"] == 0 and got["outside_box"] == 0 and got["parent_differs"] == 0
    assert cls == [WALK, WALK, WALK, WALK, WALK, WALK, NONE, WALK, BOX, SCAN]
    assert (cols[0], xmajor[0], ncells[0]) == (8, 1, 16)  # x 1.8 .. 8.2, z 4.8 .. 5.2
    assert (cols[1], xmajor[1], ncells[1]) == (8, 0, 16)
    assert (cols[2], xmajor[2]) == (7, 0) and ncells[2] <= 3 * 7  # 1.8 .. 7.2 on both axes: ties go to z
    assert (cols[3], xmajor[3]) == (7, 1) and ncells[3] <= 3 * 7
    assert (cols[4], xmajor[4], ncells[4]) == (8, 1, 16)  # x 4.3 .. 18.7, clipped to 4 .. 11
    assert (cols[5], xmajor[5], ncells[5]) == (8, 1, 16)  # x -3.2 .. 7.2, clipped to 0 .. 7
    assert (cols[7], xmajor[7]) == (12 - int(np.floor(enter - 0.2)), 1) and ncells[7] <= 3 * cols[7] and 5 <= cols[7] <= 6
    assert cols[9] == 11


@pytest.mark.parametrize("name", ["along the diagonal", "along z", "field", "from above", "strip"])
def test_each_scene_holds_the_rays_it_is_named_for(wmirror, tmp_path, name):
    """The scenes of test_slab_walk_gpu.py, whose kernels carry no counters: the mirror on each one's pixel-centre camera rays."""
    from test_plane_runs import _spheres
    from test_slab_walk_gpu import H, SCENES, W, WALK_COLUMNS

    make, classes = SCENES[name]
    t = make()
    cam = t.camera_desc()
    v = lambda f: np.array(list(getattr(cam, f)))  # noqa: E731
    py, px = np.mgrid[0:H, 0:W]
    d = v("px_origin") + px.reshape(-1, 1) * v("px_du") + py.reshape(-1, 1) * v("px_dv") - v("look_from")
    o = np.broadcast_to(v("look_from"), d.shape)
    r = np.column_stack([o, d, np.full(len(d), 0.5), np.full(len(d), -1.0)])
    assert run(wmirror, "consts")["walk_columns"] == WALK_COLUMNS
    got = run(wmirror, "check", _write(tmp_path, "s.bin", _spheres(t)), _write(tmp_path, "r.bin", r), TMIN, WALK_COLUMNS)
    cls, cols = np.array(got["cls"]), np.array(got["cols"])
    n = {"box": int((cls == 1).sum()), "walk": int((cls == 2).sum()), "over": int((cols > WALK_COLUMNS).sum())}
    print(name, n, "scan", int((cls == 3).sum()), "no cells", int((cls == 0).sum()))
    assert got["misses"] == 0 and got["twice"] == 0 and got["outside_box"] == 0
    for c in classes:
        assert n[c] >= 100, (name, c, n)
