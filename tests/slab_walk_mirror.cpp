// slab_walk_mirror.cpp — the two tiers of the cells' query (rayz_amd/csrc/slab_cells.hpp: the box of cells_query, then the walk of
// cells_walk / walk_column) on the CPU, for tests/test_slab_walk_cpu.py.  Compiled with -DRAYZ_CELLS_TUNE, so that the column cap is
// an argument (the product's constants are the defaults the program prints).
// Spheres: rows of 7 doubles {c, v, r}, a sphere's slot its row; rays: rows of 8 doubles {o, d, time, target} (target: the row of the
// member the ray was aimed at, or -1).
//   consts                                     JSON: kMaxCells, kWalkColumns, kCellCap
//   check <spheres> <rays> <tmin> <columns>    JSON: every (ray, member) pair decided by the exact f64 quadratic and held to the
//                                              entries of the tier that answered; the conditions on the walk's cells; per ray its
//                                              class (0 no cells, 1 box, 2 walk, 3 scan), its columns (0 unless the box failed on
//                                              its count alone), its cells, whether its target is among its entries and
//                                              whether its walk's major axis is x
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "../rayz_amd/csrc/slab_cells.hpp"

using namespace rayz_cells;

// cells_query as the commit before the walk had it, text for text: the helper the two tiers now share must not change an answer.
namespace parent {
inline CellBox cells_query(const CellGrid& g, const uint32_t* cells, double ox, double oy, double oz, double dx, double dy, double dz) {
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
} // namespace parent

static std::vector<double> read_doubles(const char* path) {
    std::vector<double> v;
    FILE* f = std::fopen(path, "rb");
    if (!f) {
        std::fprintf(stderr, "cannot open %s\n", path);
        std::exit(2);
    }
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    v.resize((size_t)n / sizeof(double));
    if (std::fread(v.data(), sizeof(double), v.size(), f) != v.size()) std::exit(2);
    std::fclose(f);
    return v;
}

int main(int argc, char** argv) {
    if (argc == 2 && std::string(argv[1]) == "consts") {
        std::printf("{\"max_cells\": %u, \"walk_columns\": %u, \"cell_cap\": %u}\n", kMaxCells, kWalkColumns, kCellCap);
        return 0;
    }
    if (argc != 6 || std::string(argv[1]) != "check") return 2;
    const std::vector<double> sv = read_doubles(argv[2]);
    std::vector<SphereIn> sph(sv.size() / 7);
    for (size_t i = 0; i < sph.size(); ++i) {
        for (int k = 0; k < 3; ++k) sph[i].c[k] = sv[7 * i + k], sph[i].v[k] = sv[7 * i + 3 + k];
        sph[i].r = sv[7 * i + 6];
        sph[i].slot = (uint32_t)i;
    }
    CellTable t = build_cells(sph, false, 1u);
    CellGrid& g = t.grid;
    if (!g.nx) {
        std::printf("{\"no_table\": true}\n");
        return 0;
    }
    g.list_lanes = kListLanes, g.max_cells = kMaxCells, g.walk_columns = (uint32_t)std::atoi(argv[5]), g.one_class = 0u;
    const std::vector<double> rays = read_doubles(argv[3]);
    const double tmin = std::atof(argv[4]);
    const size_t n = rays.size() / 8;
    const uint32_t* cells = t.table.data() + kTableHead;
    uint64_t hits = 0, listed_hits = 0, misses = 0, twice = 0, outside_box = 0, over_three = 0, parent_differs = 0, walk_cells = 0,
             walk_columns_sum = 0;
    std::string first_miss = "null";
    std::vector<int> cls(n), cols(n), ncells(n), target_ok(n), xmajor(n);
    for (size_t j = 0; j < n; ++j) {
        const double* o = &rays[8 * j];
        const double* d = o + 3;
        const double time = o[6];
        const long target = (long)o[7];
        const CellBox q = cells_query(g, cells, o[0], o[1], o[2], d[0], d[1], d[2]);
        const CellBox was = parent::cells_query(g, cells, o[0], o[1], o[2], d[0], d[1], d[2]);
        if (q.kind != was.kind || q.i0 != was.i0 || q.i1 != was.i1 || q.j0 != was.j0 || q.j1 != was.j1) ++parent_differs;
        std::vector<uint32_t> at; // the cells named, as j * nx + i
        cls[j] = q.kind == kNoCells ? 0 : q.kind == kSomeCells ? 1 : 3;
        cols[j] = 0;
        if (q.kind == kSomeCells)
            for (uint32_t cj = q.j0; cj <= q.j1; ++cj)
                for (uint32_t ci = q.i0; ci <= q.i1; ++ci) at.push_back(cj * g.nx + ci);
        if (q.kind == kNotListable) {
            CellStretch s;
            bool count_only;
            const CellBox b = cells_stretch(g, o[0], o[1], o[2], d[0], d[1], d[2], s, count_only);
            if (count_only) {
                const CellWalk w = cells_walk(g, cells, b, s, o[0], o[2], d[0], d[2]);
                cols[j] = (int)(w.k1 - w.k0 + 1u);
                xmajor[j] = (int)w.xmajor;
                if (w.kind == kSomeCells) {
                    cls[j] = 2;
                    walk_columns_sum += (uint64_t)cols[j];
                    for (uint32_t k = w.k0; k <= w.k1; ++k) {
                        uint32_t m0 = 1u, m1 = 0u;
                        if (!walk_column(g, b, s, w.xmajor != 0u, k, o[0], o[2], d[0], d[2], m0, m1)) continue;
                        for (uint32_t m = m0; m <= m1; ++m) {
                            const uint32_t ci = w.xmajor ? k : m, cj = w.xmajor ? m : k;
                            if (ci < b.i0 || ci > b.i1 || cj < b.j0 || cj > b.j1 || ci >= g.nx || cj >= g.nz) {
                                ++outside_box;
                                continue;
                            }
                            at.push_back(cj * g.nx + ci);
                        }
                    }
                    walk_cells += at.size();
                    if (2.0 * g.rmax * g.inv_cell <= 1.0 && at.size() > 3u * (size_t)cols[j]) ++over_three;
                }
            }
        }
        ncells[j] = (int)at.size();
        if (std::set<uint32_t>(at.begin(), at.end()).size() != at.size()) ++twice;
        std::vector<uint32_t> list;
        for (uint32_t c : at) {
            const uint32_t* rec = cells + (size_t)c * kCellWords;
            for (uint32_t e = 0; e < rec[0] && e < kCellCap; ++e) list.push_back(rec[1 + e]); // (a mutant that ignores the mark reads a count of 2^32 - 1)
        }
        target_ok[j] = -1;
        if (target >= 0) {
            target_ok[j] = 0;
            for (uint32_t x : list) target_ok[j] |= x == (uint32_t)target;
        }
        if (cls[j] == 3) continue; // such a ray scans
        const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        for (size_t i = 0; i < sph.size(); ++i) {
            if (!t.member[i]) continue; // an outlier is tested for every ray
            const SphereIn& m = sph[i];
            double e[3];
            for (int k = 0; k < 3; ++k) e[k] = m.c[k] + m.v[k] * time - o[k];
            const double hb = d[0] * e[0] + d[1] * e[1] + d[2] * e[2];
            const double cc = e[0] * e[0] + e[1] * e[1] + e[2] * e[2] - m.r * m.r;
            const double disc = hb * hb - a * cc;
            if (!(disc >= 0.0) || !((hb + std::sqrt(disc)) / a > tmin)) continue; // no root at t > tmin
            ++hits;
            bool in = false;
            for (uint32_t x : list) in = in || x == (uint32_t)i;
            listed_hits += in;
            if (!in) {
                if (!misses) first_miss = "[" + std::to_string(j) + ", " + std::to_string(i) + "]";
                ++misses;
            }
        }
    }
    std::printf("{\"rays\": %zu, \"nx\": %u, \"nz\": %u, \"cell\": %.17g, \"x0\": %.17g, \"z0\": %.17g, \"any_overflowed\": %u, \"hits\": %llu, "
                "\"listed_hits\": %llu, \"misses\": %llu, \"first_miss\": %s, \"twice\": %llu, \"outside_box\": %llu, \"over_three\": %llu, "
                "\"parent_differs\": %llu, \"walk_cells\": %llu, \"walk_columns\": %llu",
                n, g.nx, g.nz, 1.0 / g.inv_cell, g.x0, g.z0, g.any_overflowed, (unsigned long long)hits, (unsigned long long)listed_hits,
                (unsigned long long)misses, first_miss.c_str(), (unsigned long long)twice, (unsigned long long)outside_box,
                (unsigned long long)over_three, (unsigned long long)parent_differs, (unsigned long long)walk_cells,
                (unsigned long long)walk_columns_sum);
    const std::vector<int>* arrays[5] = {&cls, &cols, &ncells, &target_ok, &xmajor};
    const char* names[5] = {"cls", "cols", "ncells", "target_ok", "xmajor"};
    for (int a = 0; a < 5; ++a) {
        std::printf(", \"%s\": [", names[a]);
        for (size_t j = 0; j < n; ++j) std::printf("%s%d", j ? "," : "", (*arrays[a])[j]);
        std::printf("]");
    }
    std::printf("}\n");
    return 0;
}
