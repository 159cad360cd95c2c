// slab_cells_mirror.cpp — the library's own cell table and query (rayz_amd/csrc/slab_cells.hpp) on the CPU, for
// tests/test_slab_cells_cpu.py.  Spheres: rows of 7 doubles {c, v, r}, a sphere's slot its row; rays: rows of 7 doubles {o, d, time}.
//   hist  <spheres>                      JSON: the grid and the histogram of centres per cell (counted without the cap)
//   table <spheres> <min_members>        JSON: the grid, the outliers and every cell's record as build_cells files them
//   check <spheres> <rays> <tmin>        JSON: every (ray, member) pair decided by the exact f64 quadratic — a root at t > tmin at the
//                                        ray's time — and held to the query's cells whenever the ray is listable
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

#include "../rayz_amd/csrc/slab_cells.hpp"

using namespace rayz_cells;

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

static std::vector<SphereIn> read_spheres(const char* path) {
    const std::vector<double> v = read_doubles(path);
    std::vector<SphereIn> s(v.size() / 7);
    for (size_t i = 0; i < s.size(); ++i) {
        for (int k = 0; k < 3; ++k) s[i].c[k] = v[7 * i + k], s[i].v[k] = v[7 * i + 3 + k];
        s[i].r = v[7 * i + 6];
        s[i].slot = (uint32_t)i;
    }
    return s;
}

static void print_grid(const CellTable& t, size_t members) {
    const CellGrid& g = t.grid;
    std::printf("\"cell_cap\": %u, \"max_cells\": %u, \"nx\": %u, \"nz\": %u, \"cell\": %.17g, \"x0\": %.17g, \"z0\": %.17g, \"ylo\": %.17g, "
                "\"yhi\": %.17g, \"rmax\": %.17g, \"members\": %zu, \"n_outliers\": %u, \"any_overflowed\": %u",
                kCellCap, kMaxCells, g.nx, g.nz, g.nx ? 1.0 / g.inv_cell : 0.0, g.x0, g.z0, g.ylo, g.yhi, g.rmax, members, g.n_outliers,
                g.any_overflowed);
}

int main(int argc, char** argv) {
    if (argc < 3) return 2;
    const std::string cmd = argv[1];
    const std::vector<SphereIn> sph = read_spheres(argv[2]);
    const CellTable t = build_cells(sph, false, cmd == "table" && argc == 4 ? (uint32_t)std::atoi(argv[3]) : 1u);
    const CellGrid& g = t.grid;
    size_t members = 0;
    for (uint8_t m : t.member) members += m;
    if (cmd == "hist" && argc == 3) {
        std::map<uint32_t, uint64_t> per_cell, hist;
        for (size_t k = 0; k < sph.size(); ++k)
            if (t.member[k])
                per_cell[(uint32_t)cell_of(sph[k].c[2], g.z0, g.inv_cell) * g.nx + (uint32_t)cell_of(sph[k].c[0], g.x0, g.inv_cell)]++;
        for (const auto& kv : per_cell) hist[(uint32_t)kv.second]++;
        hist[0] = (uint64_t)g.nx * g.nz - per_cell.size();
        std::printf("{");
        print_grid(t, members);
        std::printf(", \"mean\": %.4f, \"hist\": {", g.nx ? (double)members / ((double)g.nx * g.nz) : 0.0);
        bool first = true;
        for (const auto& kv : hist) {
            std::printf("%s\"%u\": %llu", first ? "" : ", ", kv.first, (unsigned long long)kv.second);
            first = false;
        }
        std::printf("}}\n");
        return 0;
    }
    if (cmd == "table" && argc == 4) {
        std::printf("{");
        print_grid(t, members);
        std::printf(", \"member\": [");
        for (size_t k = 0; k < t.member.size(); ++k) std::printf("%s%u", k ? ", " : "", (unsigned)t.member[k]);
        std::printf("], \"table\": [");
        for (size_t k = 0; k < t.table.size(); ++k) std::printf("%s%u", k ? ", " : "", t.table[k]);
        std::printf("]}\n");
        return 0;
    }
    if (cmd == "check" && argc == 5) {
        const std::vector<double> rays = read_doubles(argv[3]);
        const double tmin = std::atof(argv[4]);
        const size_t n = rays.size() / 7;
        uint64_t hits = 0, listed_hits = 0, misses = 0, kinds[3] = {0, 0, 0}, cells_sum = 0, entries_sum = 0;
        std::string first_miss;
        if (!g.nx) {
            std::printf("{\"no_table\": true}\n");
            return 0;
        }
        const uint32_t* cells = t.table.data() + kTableHead;
        for (size_t j = 0; j < n; ++j) {
            const double* o = &rays[7 * j];
            const double* d = o + 3;
            const double time = o[6];
            const CellBox b = cells_query(g, cells, o[0], o[1], o[2], d[0], d[1], d[2]);
            kinds[b.kind]++;
            if (b.kind == kNotListable) continue; // such a ray scans
            std::vector<uint32_t> list;
            if (b.kind == kSomeCells)
                for (uint32_t cj = b.j0; cj <= b.j1; ++cj)
                    for (uint32_t ci = b.i0; ci <= b.i1; ++ci) {
                        const uint32_t* rec = cells + (size_t)(cj * g.nx + ci) * kCellWords;
                        ++cells_sum;
                        for (uint32_t e = 0; e < rec[0] && e < kCellCap; ++e) list.push_back(rec[1 + e]); // (a mutant that ignores the mark reads a count of 2^32 − 1)
                    }
            entries_sum += list.size();
            const double a = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
            for (size_t i = 0; i < sph.size(); ++i) {
                if (!t.member[i]) continue; // an outlier is tested for every ray
                const SphereIn& q = sph[i];
                double e[3];
                for (int k = 0; k < 3; ++k) e[k] = q.c[k] + q.v[k] * time - o[k];
                const double hb = d[0] * e[0] + d[1] * e[1] + d[2] * e[2];
                const double cc = e[0] * e[0] + e[1] * e[1] + e[2] * e[2] - q.r * q.r;
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
        std::printf("{\"rays\": %zu, \"no_cells\": %llu, \"some_cells\": %llu, \"not_listable\": %llu, \"hits\": %llu, \"listed_hits\": %llu, "
                    "\"misses\": %llu, \"cells_sum\": %llu, \"entries_sum\": %llu, \"first_miss\": %s}\n",
                    n, (unsigned long long)kinds[0], (unsigned long long)kinds[1], (unsigned long long)kinds[2], (unsigned long long)hits,
                    (unsigned long long)listed_hits, (unsigned long long)misses, (unsigned long long)cells_sum, (unsigned long long)entries_sum,
                    misses ? first_miss.c_str() : "null");
        return 0;
    }
    return 2;
}
