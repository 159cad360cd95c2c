// What the library's own rayz_amd/csrc/plane_runs.hpp says about how far a scan reads (tests/test_scan_feed.py):
//   scan_reach_mirror <group> <first> <end> [<first> <end> ...]   ->  {"spare_groups": 2, "reach": [...]}
#include <cstdio>
#include <cstdlib>

#include "../rayz_amd/csrc/plane_runs.hpp"

int main(int argc, char** argv) {
    if (argc < 2 || argc % 2 != 0) return 2;
    const uint32_t group = (uint32_t)std::strtoul(argv[1], nullptr, 10);
    std::printf("{\"spare_groups\": %u, \"reach\": [", rayz_plane::kScanSpareGroups);
    for (int k = 2; k + 1 < argc; k += 2)
        std::printf("%s%u", k > 2 ? ", " : "",
                    rayz_plane::scan_reach((uint32_t)std::strtoul(argv[k], nullptr, 10), (uint32_t)std::strtoul(argv[k + 1], nullptr, 10), group));
    std::printf("]}\n");
    return 0;
}
