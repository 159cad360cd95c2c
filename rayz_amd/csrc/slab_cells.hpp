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
// Columns of its major axis a walked stretch may cross (the second tier, for a box of more than kMaxCells).  DESIGN.md §6 has the
// sweep: 96 % of the headline frame's box-unlistable segments cross at most 48 columns, but a long walk holds its list phase's other
// lanes up, and past 12 columns that costs more than the scans it saves.
constexpr uint32_t kWalkColumns = 12;
// AUTO's gate for the walk: the least member count from which a launch walks (a forced ON always does).  A walk costs what its columns
// cost whatever the pool; the scan it replaces costs in proportion to the pool.  Kernel ms at 1920x1080 and 256 spp, 24 lanes, without
// the walk -> with it (profiles/r21/cell_walk/gates_walk.jsonl), by members: 1,023: 191.0 -> 256.9 | 1,932: 229.7 -> 285.3 | 4,093:
// 311.4 -> 338.6 | 6,399: 376.9 -> 377.5 | 9,999: 519.1 -> 466.0.  It breaks even at 6,399 and wins from 9,999: the gate lies between.
constexpr uint32_t kWalkMinMembers = 8192;
constexpr uint32_t kMaxOutliers = 8;
constexpr uint32_t kTableHead = kMaxOutliers;  // the table's first words: the outliers' slots; the cells' records follow, row-major (z rows)
// Lanes of a wave that must hold a listable segment before the wave runs a list phase instead of a scan (or all its live lanes, if
// fewer are live): DESIGN.md §6 has the sweeps (24 beats 16 with the walk, and without it at every grid from 16 to 40).
constexpr uint32_t kListLanes = 24;
// AUTO's gate: the least member count from which a scene takes the cells.  Measured at 1920x1080 and 256 spp, cells OFF -> ON, kernel
// ms of one launch on one DeviceScene (profiles/r18/cell_lists/gates.jsonl), by members:
//   96: 61.5 -> 110.9 | 252: 102.0 -> 135.4 | 481: 141.5 -> 153.5 | 1,023: 229.0 -> 195.6 | 1,932: 322.9 -> 236.0 | 4,093: 542.2 -> 313.3
//   | 9,999: 1,170 -> 494.8
// The first size at which ON wins (by 14.6 %, the spread 0.6 %) is the 32 x 32 grid's.  There is no samples-per-pixel gate: the table
// is built with the scene's slots and costs a launch nothing.
// Round 21 (profiles/r21/cell_walk/): with kListLanes = 24, and no walk below kWalkMinMembers, OFF -> AUTO at 1,023: 229.4 -> 184.4; OFF ->
// cells without the walk (tune build) at 1,932: 322.5 -> 229.7 | 4,093: 541.7 -> 311.4.  A FORCED ON walks at any size and loses up to
// 1,023 (141.5 -> 263.9 at 481, 229.4 -> 251.7 at 1,023; 324.2 -> 276.1 at 1,932, 542.1 -> 329.6 at 4,093).  The first winning size has not moved.
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
    uint32_t any_overflowed; // bit 0: some cell is marked kOverflowed (the builder's); bit 1, kNoWalk: this launch does not walk (the
                             // launch's, for kWalkMinMembers — in the word the kernels hold anyway: a further argument costs them spills)
#ifdef RAYZ_CELLS_TUNE // measurement builds only: the two thresholds as launch arguments (the sweeps of DESIGN.md §6)
    uint32_t list_lanes, max_cells;
    uint32_t walk_columns, one_class; // .. and the walk's: its column cap (0: no walk) and the lane rule "one class" (long counts as short)
#endif
};
#ifdef RAYZ_CELLS_TUNE
RAYZ_SC_HD uint32_t list_lanes(const CellGrid& g) { return g.list_lanes; }
RAYZ_SC_HD uint32_t max_cells(const CellGrid& g) { return g.max_cells; }
RAYZ_SC_HD uint32_t walk_columns(const CellGrid& g) { return g.walk_columns; }
RAYZ_SC_HD bool one_class(const CellGrid& g) { return g.one_class != 0u; }
#else
RAYZ_SC_HD uint32_t list_lanes(const CellGrid&) { return kListLanes; }
RAYZ_SC_HD uint32_t max_cells(const CellGrid&) { return kMaxCells; }
RAYZ_SC_HD uint32_t walk_columns(const CellGrid&) { return kWalkColumns; }
RAYZ_SC_HD bool one_class(const CellGrid&) { return false; }
#endif
constexpr uint32_t kNoWalk = 2u; // CellGrid::any_overflowed, bit 1
RAYZ_SC_HD bool overflowed_cells(const CellGrid& g) { return (g.any_overflowed & 1u) != 0u; }
RAYZ_SC_HD bool walks(const CellGrid& g) { return (g.any_overflowed & kNoWalk) == 0u && walk_columns(g) != 0u; }

// The cell coordinate of x along an axis, as a double: one subtraction, one product, one floor, each monotone in x under rounding —
// so lo <= cx <= hi in f64 gives cell_of(lo) <= cell_of(cx) <= cell_of(hi), and a centre is filed with this very function.
RAYZ_SC_HD double cell_of(double x, double x0, double inv_cell) { return floor((x - x0) * inv_cell); }

enum : uint32_t { kNoCells = 0, kSomeCells = 1, kNotListable = 2 };
constexpr uint32_t kWalkMajorX = 4u; // cells_stretch's own flag beside kNotListable: the walk's major axis is x (cells_query strips it)
struct CellBox {
    uint32_t kind;
    uint32_t i0, i1, j0, j1; // kSomeCells: the cells [i0 .. i1] x [j0 .. j1], inside the grid
};

RAYZ_SC_HD double min2(double a, double b) { return a < b ? a : b; }
RAYZ_SC_HD double max2(double a, double b) { return a > b ? a : b; }

// The stretch of the ray inside the slab and its xz box, the part the box and the walk share.  `count_only`: a kNotListable answer
// has no other reason than the box's cell count (b's ranges are then the clipped box, and the walk may be asked).
struct CellStretch {
    double t0, t1; // the stretch, t0 >= 0
    double px, pz; // the box's dilations
};
RAYZ_SC_HD CellBox cells_stretch(const CellGrid& g, double ox, double oy, double oz, double dx, double dy, double dz, CellStretch& s,
                                 bool& count_only) {
    CellBox b;
    b.kind = kNotListable;
    b.i0 = b.i1 = b.j0 = b.j1 = 0u;
    count_only = false;
    s.t0 = s.t1 = s.px = s.pz = 0.0;
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
    s.t0 = t0, s.t1 = t1, s.px = px, s.pz = pz;
    if ((uint64_t)(b.i1 - b.i0 + 1u) * (uint64_t)(b.j1 - b.j0 + 1u) > max_cells(g)) {
        // the major axis is chosen by the index ranges BEFORE the clip (a stretch that leaves the grid keeps its direction's axis)
        count_only = true;
        b.kind = kNotListable | (fi1 - fi0 > fj1 - fj0 ? kWalkMajorX : 0u);
        return b;
    }
    b.kind = kSomeCells;
    return b;
}

RAYZ_SC_HD bool box_overflowed(const CellGrid& g, const uint32_t* cells, const CellBox& b) {
    for (uint32_t j = b.j0; j <= b.j1; ++j)
        for (uint32_t i = b.i0; i <= b.i1; ++i)
            if (cells[(size_t)(j * g.nx + i) * kCellWords] == kOverflowed) return true;
    return false;
}

// The cells whose members the ray o + t·d can meet at some t > 0 (any time of the shutter).  `cells`: the table's records (behind its
// head), read only where some cell is overflowed.  The proof is DESIGN.md §4.22.
RAYZ_SC_HD CellBox cells_query(const CellGrid& g, const uint32_t* cells, double ox, double oy, double oz, double dx, double dy, double dz) {
    CellStretch s;
    bool count_only;
    CellBox b = cells_stretch(g, ox, oy, oz, dx, dy, dz, s, count_only);
    if (b.kind != kSomeCells) {
        b.kind &= 3u;
        return b;
    }
    if (overflowed_cells(g) && box_overflowed(g, cells, b)) b.kind = kNotListable;
    return b;
}

// ---- the walk: the second tier, asked only where the box fails on its cell count ----
// The MAJOR axis is the one of x / z with the wider index range (ties: z); a COLUMN is one index of it.  Column k's cells are those
// under the part of the stretch whose major coordinate lies in the column's interval dilated by p: the minor coordinate at that
// sub-stretch's two ends, dilated likewise, through cell_of.  Columns are disjoint, so no cell is named twice, and every range is
// clipped to the box's, so no cell lies outside it.
struct CellWalk {
    uint32_t kind;   // kNotListable, or kSomeCells: the columns [k0 .. k1] (inside the grid)
    uint32_t xmajor; // the major axis is x (a column is an i, its range runs over j), else z
    uint32_t k0, k1;
};

// Column k's minor range [m0 .. m1] for the box b and its stretch s; false: the column names no cell.
RAYZ_SC_HD bool walk_column(const CellGrid& g, const CellBox& b, const CellStretch& s, bool xmajor, uint32_t k, double ox, double oz,
                            double dx, double dz, uint32_t& m0, uint32_t& m1) {
    const double om = xmajor ? ox : oz, dm = xmajor ? dx : dz, on = xmajor ? oz : ox, dn = xmajor ? dz : dx;
    const double g0m = xmajor ? g.x0 : g.z0, g0n = xmajor ? g.z0 : g.x0;
    const double cell = 1.0 / g.inv_cell; // exact: a power of two
    // the column's interval.  A member filed under k has its centre in [e0, e1) up to the rounding of cell_of's subtraction and of
    // the two edges (kRel·(|x0| + |e0| + |e1|)); an accepted root lies within the box's px of the centre; the two quotients below
    // err by a few 2^-53 of |om| + |e|, which the kRel share of pm outweighs by 10^6 — so the computed sub-stretch holds the root's t.
    const double e0 = g0m + (double)k * cell, e1 = g0m + ((double)k + 1.0) * cell;
    const double pm = (xmajor ? s.px : s.pz) + kRel * (fabs(om) + fabs(g0m) + fabs(e0) + fabs(e1));
    double s0 = s.t0, s1 = s.t1;
    double band = INFINITY, ba = 0.0, bb = 0.0; // (a stretch across the major axis has no band)
    if (dm != 0.0) {
        const double inv = 1.0 / dm;
        const double ta = ((e0 - pm) - om) * inv, tb = ((e1 + pm) - om) * inv;
        s0 = max2(s0, min2(ta, tb)), s1 = min2(s1, max2(ta, tb)); // clipped to the stretch: never a cell outside the box's reach
        // The BAND, a second bound on the same centres.  The root X lies on the line minor = on + (major − om)·sl, and within rho =
        // |r| + eps of the centre C in the plane (the distance §4.22 step 2 bounds is Euclidean), so by Cauchy-Schwarz C.minor is
        // within rho·sqrt(1 + sl²) <= rho·(1 + sl²/2) of the line's minor coordinate at C.major, which lies in [e0, e1].
        const double sl = dn * inv;
        ba = on + (e0 - om) * sl, bb = on + (e1 - om) * sl;
        band = (1.0 + 0.5 * sl * sl) * ((xmajor ? s.pz : s.px) + kRel * (fabs(on) + fabs(ba) + fabs(bb))) +
               kRel * (1.0 + fabs(sl)) * (fabs(om) + fabs(g0m) + fabs(e0) + fabs(e1));
    }
    if (!(s0 <= s1)) return false; // the stretch does not reach this column
    // the minor coordinate is linear in t: at the root it lies between its values at the sub-stretch's ends (one product, one sum each)
    const double na = on + s0 * dn, nb = on + s1 * dn;
    const double pn = (xmajor ? s.pz : s.px) + kRel * (fabs(on) + fabs(na) + fabs(nb));
    double f0 = cell_of(min2(na, nb) - pn, g0n, g.inv_cell), f1 = cell_of(max2(na, nb) + pn, g0n, g.inv_cell);
    if (band < INFINITY) // both ranges hold the centre's cell (cell_of is monotone): so does their intersection
        f0 = max2(f0, cell_of(min2(ba, bb) - band, g0n, g.inv_cell)), f1 = min2(f1, cell_of(max2(ba, bb) + band, g0n, g.inv_cell));
    const double lo = (double)(xmajor ? b.j0 : b.i0), hi = (double)(xmajor ? b.j1 : b.i1);
    if (!(f1 >= lo) || !(f0 <= hi) || !(f0 <= f1)) return false; // (also a NaN)
    m0 = (uint32_t)max2(f0, lo), m1 = (uint32_t)min2(f1, hi);
    return true;
}

// The walk of a ray whose box `b` (of cells_stretch) failed on its cell count alone.
RAYZ_SC_HD CellWalk cells_walk(const CellGrid& g, const uint32_t* cells, const CellBox& b, const CellStretch& s, double ox, double oz,
                               double dx, double dz) {
    CellWalk w;
    w.kind = kNotListable;
    w.xmajor = (b.kind & kWalkMajorX) ? 1u : 0u;
    w.k0 = w.xmajor ? b.i0 : b.j0, w.k1 = w.xmajor ? b.i1 : b.j1; // the box's range, clipped to the grid already
    if (w.k1 - w.k0 + 1u > walk_columns(g)) return w;
    if (overflowed_cells(g))
        for (uint32_t k = w.k0; k <= w.k1; ++k) {
            uint32_t m0, m1;
            if (!walk_column(g, b, s, w.xmajor != 0u, k, ox, oz, dx, dz, m0, m1)) continue;
            for (uint32_t m = m0; m <= m1; ++m)
                if (cells[(size_t)(w.xmajor ? m * g.nx + k : k * g.nx + m) * kCellWords] == kOverflowed) return w;
        }
    w.kind = kSomeCells;
    return w;
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
