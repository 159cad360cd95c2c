// slab_cells.hpp — which spheres a ray can hit at all, read off a grid of cells under the ray's stretch inside the slab that holds
// the scene's small spheres.  The MEMBERS — spheres that do not move in x or z and are no wider than a cell — live
// between two heights for the whole shutter; a ray meets one only while its own y lies between them, and the xz box of that stretch,
// dilated by the largest member radius, names the cells whose centres it can reach.  Everything else is an OUTLIER (at most
// kMaxOutliers) and is tested for every ray.  The trace kernels compiled with RAYZ_TRACE_KERNEL_CELLS resolve such a segment from the
// outliers and the cells' slots (narrow_eval decides, as it does behind the scan) instead of scanning the whole flat list.
// The query only has to be a SUPERSET: it is f64 throughout, host and device, on the ray as narrow_eval gets it.
// Also compiled by the host compiler alone (tests/slab_cells_mirror.cpp).
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RAYZ_SC_HD __host__ __device__ __forceinline__
#else
#define RAYZ_SC_HD inline
#endif

namespace rayz_cells {

// kCellCap: slots a cell's record holds; a cell with more centres is marked kOverflowed and a ray whose box touches it scans.
// The headline scene and config 2 need only ONE (tests/slab_cells_mirror.cpp `hist`, DESIGN.md §6: the cell comes out as 1.0, the
// grid's origin is a multiple of it, and the generator puts at most one centre in a unit square of its lattice: no cell of either
// holds two).  Three is what a record of one 16-byte load has room for, and what a pool WITHOUT a lattice needs: at a mean
// occupancy of one, Poisson leaves 8 % of the cells with three centres or more, but 1.9 % with four or more.
constexpr uint32_t kCellCap = 3;
constexpr uint32_t kCellWords = kCellCap + 1u; // a record: the count, then the slots
constexpr uint32_t kOverflowed = 0xffffffffu;  // .. or this for a fuller cell
constexpr uint32_t kMaxCells = 12;             // cells a listable ray's box may cover (DESIGN.md §6 has the GPU histogram)
constexpr uint32_t kMaxOutliers = 8;
constexpr uint32_t kTableHead = kMaxOutliers;  // the table's first words: the outliers' slots; the cells' records follow, row-major (z rows)
// Lanes of a wave that must hold a listable segment before the wave runs a list phase instead of a scan (or all its live lanes, if
// fewer are live): DESIGN.md §6 has the sweep.
constexpr uint32_t kListLanes = 16;
// AUTO's gate: the least member count from which a scene takes the cells.  Measured at 1920x1080 and 256 spp, cells OFF -> ON, kernel
// ms of one launch on one DeviceScene (profiles/r18/cell_lists/gates.jsonl), by members:
//   96: 61.5 -> 110.9 | 252: 102.0 -> 135.4 | 481: 141.5 -> 153.5 | 1,023: 229.0 -> 195.6 | 1,932: 322.9 -> 236.0 | 4,093: 542.2 -> 313.3
//   | 9,999: 1,170 -> 494.8
// The first size at which ON wins (by 14.6 %, the spread 0.6 %) is the 32 x 32 grid's.  There is no samples-per-pixel gate: the table
// is built with the scene's slots and costs a launch nothing.
constexpr uint32_t kCellsMinMembers = 1023;
constexpr uint32_t kMaxGridSide = 4096; // cells per side at most: the table stays below 2^24 records

// Margins.  kRel: the f64 roundings of this file's own arithmetic (each a few 2^-53 relative).  kEvalRel: narrow_eval's rounded
// discriminant and root, in the style of beam_may_hit's slack2 — a root it accepts lies within sqrt(r² + (kEvalRel·Q)²) <= |r| +
// kEvalRel·Q of the centre, Q bounding the lengths that enter its sums (1e-12 of their squares is a thousand times the rounding).
constexpr double kRel = 1e-9, kEvalRel = 1e-6;

// The grid, as the kernels hold it (wave-uniform: kernel arguments).  nx = 0: the scene has no cells.
struct CellGrid {
    double ylo, yhi;         // the slab: the hull of cy ± |r| and cy + vy ± |r| over the members
    double x0, z0, inv_cell; // cell (i, j) covers x0 + i·cell <= x < x0 + (i + 1)·cell, z0 + j·cell <= z < ..
    double rmax;             // the largest |r| of a member
    double extent;           // >= |cx| + |cy| + |cz| + |vy| + |r| of every member
    uint32_t nx, nz;
    uint32_t n_outliers;
    uint32_t any_overflowed; // some cell is marked kOverflowed
#ifdef RAYZ_CELLS_TUNE // measurement builds only: the two thresholds as launch arguments (the sweeps of DESIGN.md §6)
    uint32_t list_lanes, max_cells;
#endif
};
#ifdef RAYZ_CELLS_TUNE
RAYZ_SC_HD uint32_t list_lanes(const CellGrid& g) { return g.list_lanes; }
RAYZ_SC_HD uint32_t max_cells(const CellGrid& g) { return g.max_cells; }
#else
RAYZ_SC_HD uint32_t list_lanes(const CellGrid&) { return kListLanes; }
RAYZ_SC_HD uint32_t max_cells(const CellGrid&) { return kMaxCells; }
#endif

// The cell coordinate of x along an axis, as a double: one subtraction, one product, one floor, each monotone in x under rounding —
// so lo <= cx <= hi in f64 gives cell_of(lo) <= cell_of(cx) <= cell_of(hi), and a centre is filed with this very function.
RAYZ_SC_HD double cell_of(double x, double x0, double inv_cell) { return floor((x - x0) * inv_cell); }

enum : uint32_t { kNoCells = 0, kSomeCells = 1, kNotListable = 2 };
struct CellBox {
    uint32_t kind;
    uint32_t i0, i1, j0, j1; // kSomeCells: the cells [i0 .. i1] x [j0 .. j1], inside the grid
};

RAYZ_SC_HD double min2(double a, double b) { return a < b ? a : b; }
RAYZ_SC_HD double max2(double a, double b) { return a > b ? a : b; }

// The cells whose members the ray o + t·d can meet at some t > 0 (any time of the shutter).  `cells`: the table's records (behind its
// head), read only where some cell is overflowed.  The proof is DESIGN.md §4.22.
RAYZ_SC_HD CellBox cells_query(const CellGrid& g, const uint32_t* cells, double ox, double oy, double oz, double dx, double dy, double dz) {
    CellBox b;
    b.kind = kNotListable;
    b.i0 = b.i1 = b.j0 = b.j1 = 0u;
    if (!(dy != 0.0)) return b; // a ray along the slab (or a NaN)
    // what narrow_eval's rounding can add to a member's radius for this origin
    const double eps = kEvalRel * 2.0 * (fabs(ox) + fabs(oy) + fabs(oz) + g.extent);
    // 1. the stretch of t in which the ray's y is inside the slab, widened by eps and by the rounding of the two quotients
    const double my = eps + kRel * (fabs(oy) + fabs(g.ylo) + fabs(g.yhi));
    const double inv = 1.0 / dy;
    const double ta = ((g.ylo - my) - oy) * inv, tb = ((g.yhi + my) - oy) * inv;
    double t0 = min2(ta, tb);
    const double t1 = max2(ta, tb);
    if (t1 < 0.0) {
        b.kind = kNoCells; // the slab lies behind the origin
        return b;
    }
    if (!(t1 >= 0.0)) return b; // (NaN)
    t0 = t0 > 0.0 ? t0 : 0.0;   // only t >= 0 counts
    // 2. the xz box of that stretch, dilated by the largest radius, eps and the rounding of the four end points
    const double xa = ox + t0 * dx, xb = ox + t1 * dx, za = oz + t0 * dz, zb = oz + t1 * dz;
    const double px = g.rmax + eps + kRel * (fabs(ox) + fabs(xa) + fabs(xb) + g.rmax);
    const double pz = g.rmax + eps + kRel * (fabs(oz) + fabs(za) + fabs(zb) + g.rmax);
    // 3. cell index ranges, clipped to the grid
    const double fi0 = cell_of(min2(xa, xb) - px, g.x0, g.inv_cell), fi1 = cell_of(max2(xa, xb) + px, g.x0, g.inv_cell);
    const double fj0 = cell_of(min2(za, zb) - pz, g.z0, g.inv_cell), fj1 = cell_of(max2(za, zb) + pz, g.z0, g.inv_cell);
    const double big = 1e15; // beyond it (or non-finite: a stretch that does not end) the indices mean nothing
    if (!(fabs(fi0) < big) || !(fabs(fi1) < big) || !(fabs(fj0) < big) || !(fabs(fj1) < big)) return b;
    const double lx = (double)g.nx - 1.0, lz = (double)g.nz - 1.0;
    if (fi1 < 0.0 || fi0 > lx || fj1 < 0.0 || fj0 > lz) {
        b.kind = kNoCells; // the stretch passes beside the grid
        return b;
    }
    b.i0 = (uint32_t)max2(fi0, 0.0), b.i1 = (uint32_t)min2(fi1, lx);
    b.j0 = (uint32_t)max2(fj0, 0.0), b.j1 = (uint32_t)min2(fj1, lz);
    if ((uint64_t)(b.i1 - b.i0 + 1u) * (uint64_t)(b.j1 - b.j0 + 1u) > max_cells(g)) return b;
    if (g.any_overflowed)
        for (uint32_t j = b.j0; j <= b.j1; ++j)
            for (uint32_t i = b.i0; i <= b.i1; ++i)
                if (cells[(size_t)(j * g.nx + i) * kCellWords] == kOverflowed) return b;
    b.kind = kSomeCells;
    return b;
}

} // namespace rayz_cells

// ---- the builder (host code) ----
#include <vector>

namespace rayz_cells {

// One sphere of the pool as the builder reads it: the pool's own f64 values and the slot the scan numbers it by.
struct SphereIn {
    double c[3], v[3], r;
    uint32_t slot;
};
struct CellTable {
    CellGrid grid{};             // grid.nx = 0: no cells (and `table` is empty)
    std::vector<uint32_t> table; // [kTableHead outlier slots][nx · nz records of kCellWords]
    std::vector<uint8_t> member; // per input sphere: filed in a cell (else an outlier)
};

inline bool finite7(const SphereIn& s) {
    for (int k = 0; k < 3; ++k)
        if (!(fabs(s.c[k]) < 1e300) || !(fabs(s.v[k]) < 1e300)) return false;
    return fabs(s.r) < 1e300;
}

// The scene's table, or none: with a triangle, with more than kMaxOutliers outliers, with fewer than `min_members` members (AUTO's
// gate; at least one), or with a grid beyond kMaxGridSide cells a side.
inline CellTable build_cells(const std::vector<SphereIn>& s, bool any_triangle, uint32_t min_members) {
    CellTable t;
    t.member.assign(s.size(), 0);
    if (any_triangle || s.empty()) return t;
    // the cell: a power of two near sqrt(area / count) of the spheres that could be members at any cell size (mean occupancy about one)
    double lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
    size_t cand = 0;
    for (const SphereIn& q : s)
        if (finite7(q) && q.v[0] == 0.0 && q.v[2] == 0.0) {
            ++cand;
            lo[0] = min2(lo[0], q.c[0]), hi[0] = max2(hi[0], q.c[0]), lo[1] = min2(lo[1], q.c[2]), hi[1] = max2(hi[1], q.c[2]);
        }
    if (!cand) return t;
    const double side = sqrt(max2(hi[0] - lo[0], 0.0) * max2(hi[1] - lo[1], 0.0) / (double)cand);
    double cell = side > 0.0 && side < 1e300 ? exp2(floor(log2(side) + 0.5)) : 1.0;
    cell = min2(max2(cell, 0x1p-20), 0x1p20);
    // members, and the grid over their centres (its origin a multiple of the cell)
    std::vector<uint32_t> outliers;
    size_t members = 0;
    CellGrid& g = t.grid;
    g.ylo = INFINITY, g.yhi = -INFINITY, g.rmax = 0.0, g.extent = 0.0;
    lo[0] = lo[1] = INFINITY, hi[0] = hi[1] = -INFINITY;
    for (size_t k = 0; k < s.size(); ++k) {
        const SphereIn& q = s[k];
        const double ra = fabs(q.r);
        if (!(finite7(q) && q.v[0] == 0.0 && q.v[2] == 0.0 && ra <= 0.5 * cell)) {
            outliers.push_back(q.slot);
            continue;
        }
        t.member[k] = 1;
        ++members;
        g.ylo = min2(g.ylo, min2(q.c[1], q.c[1] + q.v[1]) - ra), g.yhi = max2(g.yhi, max2(q.c[1], q.c[1] + q.v[1]) + ra);
        g.rmax = max2(g.rmax, ra);
        g.extent = max2(g.extent, fabs(q.c[0]) + fabs(q.c[1]) + fabs(q.c[2]) + fabs(q.v[1]) + ra);
        lo[0] = min2(lo[0], q.c[0]), hi[0] = max2(hi[0], q.c[0]), lo[1] = min2(lo[1], q.c[2]), hi[1] = max2(hi[1], q.c[2]);
    }
    const uint32_t least = min_members > 1u ? min_members : 1u;
    auto none = [&] {
        t.member.assign(s.size(), 0);
        t.grid = CellGrid{};
        t.table.clear();
        return t;
    };
    if (outliers.size() > kMaxOutliers || members < least) return none();
    g.inv_cell = 1.0 / cell; // exact: a power of two
    g.x0 = floor(lo[0] * g.inv_cell) * cell, g.z0 = floor(lo[1] * g.inv_cell) * cell;
    const double fx = cell_of(hi[0], g.x0, g.inv_cell), fz = cell_of(hi[1], g.z0, g.inv_cell);
    if (!(fx >= 0.0 && fx < (double)kMaxGridSide && fz >= 0.0 && fz < (double)kMaxGridSide)) return none();
    if (!(cell_of(lo[0], g.x0, g.inv_cell) >= 0.0) || !(cell_of(lo[1], g.z0, g.inv_cell) >= 0.0)) return none(); // (an origin the rounding lifted)
    g.nx = (uint32_t)fx + 1u, g.nz = (uint32_t)fz + 1u;
    g.n_outliers = (uint32_t)outliers.size();
    t.table.assign((size_t)kTableHead + (size_t)g.nx * g.nz * kCellWords, 0u);
    for (size_t k = 0; k < outliers.size(); ++k) t.table[k] = outliers[k];
    for (size_t k = 0; k < s.size(); ++k)
        if (t.member[k]) {
            const uint32_t i = (uint32_t)cell_of(s[k].c[0], g.x0, g.inv_cell), j = (uint32_t)cell_of(s[k].c[2], g.z0, g.inv_cell);
            uint32_t* rec = &t.table[(size_t)kTableHead + (size_t)(j * g.nx + i) * kCellWords];
            if (rec[0] == kOverflowed) continue;
            if (rec[0] == kCellCap) {
                rec[0] = kOverflowed;
                g.any_overflowed = 1u;
            } else {
                rec[1u + rec[0]] = s[k].slot;
                rec[0]++;
            }
        }
    return t;
}

} // namespace rayz_cells
