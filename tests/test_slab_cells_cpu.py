"""The slab's cells: the table `build_cells` and the query `cells_query` of rayz_amd/csrc/slab_cells.hpp, compiled
into a stand-alone host program (tests/slab_cells_mirror.cpp).

Superset: per pool 20,000 rays — origins inside the slab, above it, below it, 3·10⁴ away and on member surfaces; directions aimed at
members and random, a tenth of them nearly along the slab, some exactly along it; lengths 0.05, 1 and 10 (a scattered, a reflected and
a camera ray's); times in [0, 1], a tenth at 0 or 1.  The mirror decides every (ray, member) pair with the exact f64 quadratic — a root
at t > tmin at the ray's time — and every hit of a listable ray must be in the query's cells.  Zero misses, and the cells, not the
fallback, must have answered.  Pools: the headline scene's and config 2's; negative radii; a slab at height ±0 and one at 3·10⁴; a
cell with kCellCap centres next to one with kCellCap + 1; centres on cell borders and on the grid's edge.

Table: every record equals a brute-force filing done here.

Mutations of the header, each run once against this file and each failing it (not committed):
  * the dilation dropped (rmax left out of px and pz in cells_query): all 7 pools fail the superset test (5 to 1,723 misses);
  * the slab taken at time 0 only (cy + vy left out of ylo / yhi in build_cells): 6 pools fail it (46 to 2,447 misses; slab_at_zero
    has no mover), and the table test fails on yhi;
  * the t >= 0 clamp dropped (t0 left negative): no miss — the box only grows, correctness never rested on the clamp — but headline
    and negative_radii fall below the stated floor of listable rays (53 % and 51 %), which is what the clamp is for;
  * the overflow mark ignored (the any_overflowed loop skipped): cap_and_cap_plus_one and borders_and_edge fail (52 and 146 misses).
kRel and kEvalRel are NOT reached: with both set to 0 this file still passes, as r15's f32 margins were not reached by its test.
An f64 rounding is far smaller than anything 20,000 random rays get to; those two margins rest on §4.22's steps, not on a test."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from rayz_amd import tracer
from test_plane_runs import _spheres, _write

HERE = os.path.dirname(os.path.abspath(__file__))
N_RAYS = 20_000
CAP, MAX_CELLS, MAX_OUTLIERS = 3, 12, 8  # slab_cells.hpp: kCellCap, kMaxCells, kMaxOutliers
TMIN = 1e-3


@pytest.fixture(scope="module")
def cmirror(tmp_path_factory):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("no g++")
    exe = str(tmp_path_factory.mktemp("slab_cells") / "slab_cells_mirror")
    subprocess.run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "slab_cells_mirror.cpp")],
                   check=True, capture_output=True, timeout=300)
    return exe


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return json.loads(r.stdout)


def _lattice(rng, n, y=0.2, r=0.2, neg=False, offset=(0.0, 0.0, 0.0)):
    """n x n small spheres, one per unit square, a third of them y-moving; the ground and a big sphere as outliers."""
    rows = [[0.0 + offset[0], -1000.0 + offset[1], 0.0 + offset[2], 0, 0, 0, 1000.0], [1.0 + offset[0], 1.0 + offset[1], offset[2], 0, 0, 0, 1.0]]
    for a in range(n):
        for b in range(n):
            vy = float(rng.uniform(0.0, 0.5)) if (a + b) % 3 == 0 else 0.0
            rr = -r if neg and (a + b) % 2 else r
            rows.append([a + 0.9 * rng.uniform() + offset[0], y + offset[1], b + 0.9 * rng.uniform() + offset[2], 0, vy, 0, rr])
    return np.array(rows, dtype=np.float64)


def pool(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "headline":
        return _spheres(tracer.randomBouncing(64, -50, 50, seed=42))
    if name == "config2":
        return _spheres(tracer.randomBouncing(64, seed=42))
    if name == "negative_radii":  # hollow members, random heights and radii
        s = _lattice(rng, 14, neg=True)
        s[2:, 1] = rng.uniform(-0.5, 0.8, len(s) - 2)
        s[2:, 6] *= rng.uniform(0.3, 1.0, len(s) - 2)
        return s
    if name == "slab_at_zero":  # heights at +0 and -0, no mover: the slab is [-r, r]
        s = _lattice(rng, 12, y=0.0)
        s[2:, 4] = 0.0
        s[2::2, 1] = -0.0
        return s
    if name == "slab_at_3e4":
        return _lattice(rng, 12, offset=(0.0, 3.0e4, 0.0))
    if name == "cap_and_cap_plus_one":  # cell (3, 3) holds kCellCap centres, cell (4, 3) kCellCap + 1
        s = _lattice(rng, 12, r=0.1)
        extra = [[3.2 + 0.2 * k, 0.2, 3.5, 0, 0, 0, 0.1] for k in range(CAP - 1)] + [[4.2 + 0.15 * k, 0.2, 3.5, 0, 0, 0, 0.1] for k in range(CAP)]
        return np.vstack([s, np.array(extra, dtype=np.float64)])
    if name == "borders_and_edge":  # centres exactly on cell borders, on the grid's first and last lines
        s = _lattice(rng, 10)
        s[2:, 0] = np.round(s[2:, 0])
        s[2::2, 2] = np.round(s[2::2, 2])
        return s
    raise KeyError(name)


POOLS = ["headline", "config2", "negative_radii", "slab_at_zero", "slab_at_3e4", "cap_and_cap_plus_one", "borders_and_edge"]


def members_of(s, cell):
    return (s[:, 3] == 0) & (s[:, 5] == 0) & (np.abs(s[:, 6]) <= 0.5 * cell)


def rays(rng, s, grid, n):
    """(n, 7): o, d, time (the module docstring has the mix)."""
    m = s[members_of(s, grid["cell"])]
    ylo, yhi = grid["ylo"], grid["yhi"]
    xlo, xhi, zlo, zhi = m[:, 0].min() - 2, m[:, 0].max() + 2, m[:, 2].min() - 2, m[:, 2].max() + 2
    time = rng.uniform(0.0, 1.0, n)
    time[::10] = rng.choice([0.0, 1.0], len(time[::10]))
    o = np.empty((n, 3))
    o[:, 0], o[:, 2] = rng.uniform(xlo, xhi, n), rng.uniform(zlo, zhi, n)
    kind = rng.integers(0, 8, n)
    o[:, 1] = rng.uniform(ylo, yhi, n)                                      # 0, 1: inside the slab
    above, below, far, surf = (kind == 2) | (kind == 3), kind == 4, kind == 5, kind >= 6
    o[above, 1] = yhi + rng.uniform(0.0, 5.0, above.sum())
    o[below, 1] = ylo - rng.uniform(0.0, 3.0, below.sum())
    o[far] += rng.choice([-3.0e4, 0.0, 3.0e4], (far.sum(), 3))
    pick = m[rng.integers(0, len(m), n)]
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    centre = pick[:, :3] + pick[:, 3:6] * time[:, None]
    o[surf] = (centre + np.abs(pick[:, 6:7]) * u)[surf]
    d = rng.normal(size=(n, 3))
    aimed = rng.uniform(size=n) < 0.5
    d[aimed] = (centre + 0.9 * np.abs(pick[:, 6:7]) * rng.uniform(-1, 1, (n, 3)) - o)[aimed]
    d /= np.maximum(np.linalg.norm(d, axis=1, keepdims=True), 1e-300)
    graze = rng.uniform(size=n) < 0.1
    d[graze, 1] *= 1e-3
    d[::97, 1] = 0.0
    d *= rng.choice([0.05, 1.0, 10.0], (n, 1))
    return np.column_stack([o, d, time])


@pytest.mark.parametrize("name", POOLS)
def test_every_member_a_listable_ray_hits_is_in_its_cells(cmirror, tmp_path, name):
    s = pool(name)
    sp = _write(tmp_path, "s.bin", s)
    grid = _run(cmirror, "hist", sp)
    assert grid["nx"] > 0 and grid["members"] == int(members_of(s, grid["cell"]).sum())
    if name != "borders_and_edge":  # (centres rounded to the lattice's corners: up to four in a cell)
        assert (grid["any_overflowed"] == 1) == (name == "cap_and_cap_plus_one")
    if name in ("headline", "config2"):  # what kCellCap was chosen from
        print(name, "occupancy", grid["hist"], "cell", grid["cell"])
        assert grid["cell"] == 1.0 and max(map(int, grid["hist"])) <= CAP
    rp = _write(tmp_path, "r.bin", rays(np.random.default_rng(11), s, grid, N_RAYS))
    got = _run(cmirror, "check", sp, rp, TMIN)
    print(name, got)
    assert got["rays"] == N_RAYS
    assert got["misses"] == 0, got
    assert got["listed_hits"] >= 2_000, got  # the cells answered ..
    assert got["some_cells"] + got["no_cells"] >= 0.55 * N_RAYS, got  # .. for most rays (the t >= 0 clamp's work: without it about a third)
    assert got["not_listable"] >= 100, got  # .. and the fallback was met as well


def test_the_table_equals_a_brute_force_filing(cmirror, tmp_path):
    for name in POOLS[1:]:
        s = pool(name)
        got = _run(cmirror, "table", _write(tmp_path, "s.bin", s), 1)
        cand = (s[:, 3] == 0) & (s[:, 5] == 0)
        side = np.sqrt((s[cand, 0].max() - s[cand, 0].min()) * (s[cand, 2].max() - s[cand, 2].min()) / cand.sum())
        cell = 2.0 ** np.floor(np.log2(side) + 0.5)
        mem = members_of(s, cell)
        assert got["cell"] == cell and got["member"] == mem.astype(int).tolist(), name
        m = s[mem]
        ra = np.abs(m[:, 6])
        assert got["ylo"] == (np.minimum(m[:, 1], m[:, 1] + m[:, 4]) - ra).min() and got["yhi"] == (np.maximum(m[:, 1], m[:, 1] + m[:, 4]) + ra).max()
        assert got["rmax"] == ra.max()
        x0, z0 = np.floor(m[:, 0].min() / cell) * cell, np.floor(m[:, 2].min() / cell) * cell
        nx, nz = int(np.floor((m[:, 0].max() - x0) / cell)) + 1, int(np.floor((m[:, 2].max() - z0) / cell)) + 1
        assert (got["x0"], got["z0"], got["nx"], got["nz"]) == (x0, z0, nx, nz), name
        table = got["table"]
        assert len(table) == MAX_OUTLIERS + nx * nz * (CAP + 1)
        assert table[:got["n_outliers"]] == np.flatnonzero(~mem).tolist() and not any(table[got["n_outliers"]:MAX_OUTLIERS])
        filed = {}
        for k in np.flatnonzero(mem):
            filed.setdefault((int(np.floor((s[k, 0] - x0) / cell)), int(np.floor((s[k, 2] - z0) / cell))), []).append(int(k))
        overflowed = 0
        for j in range(nz):
            for i in range(nx):
                rec = table[MAX_OUTLIERS + (j * nx + i) * (CAP + 1):][:CAP + 1]
                want = filed.get((i, j), [])
                if len(want) > CAP:
                    assert rec[0] == 0xFFFFFFFF, (name, i, j)
                    overflowed += 1
                else:
                    assert rec[0] == len(want) and rec[1:1 + len(want)] == want, (name, i, j, rec, want)
        assert got["any_overflowed"] == (overflowed > 0)
        if name == "cap_and_cap_plus_one":
            assert overflowed == 1 and len(filed[(3, 3)]) == CAP and len(filed[(4, 3)]) == CAP + 1


def test_scenes_without_cells(cmirror, tmp_path):
    """More than kMaxOutliers outliers, and fewer members than the gate asks for: no table."""
    s = _lattice(np.random.default_rng(5), 6)
    # the ground and seven spheres wider than half a cell (the cell comes out as 4: the lattice's unit sphere is a member there)
    big = np.array([[20.0 + 7 * k, 3.0, 0.0, 0, 0, 0, 3.0] for k in range(MAX_OUTLIERS - 1)])
    got = _run(cmirror, "table", _write(tmp_path, "a.bin", np.vstack([s, big])), 1)
    assert got["nx"] > 0 and got["cell"] == 4.0 and got["n_outliers"] == MAX_OUTLIERS and got["members"] == 37
    more = np.vstack([s, big, [[30.0, 1.0, 0.0, 0.1, 0, 0, 0.2]]])  # .. a ninth: a sphere moving in x
    assert _run(cmirror, "table", _write(tmp_path, "b.bin", more), 1)["nx"] == 0
    assert _run(cmirror, "table", _write(tmp_path, "c.bin", s), 36)["nx"] > 0  # the lattice alone: 36 members under a cell of 1
    assert _run(cmirror, "table", _write(tmp_path, "c.bin", s), 37)["nx"] == 0
