// bvh_layout_mirror.cpp — what the device is handed for a pool: the library's own builder (rayz_amd/csrc/bvh_build.hpp) run on
// a scene's spheres and triangles for every (peel_oversized, sah), and the oversized hittables' descriptors restated from its
// `big` list as upload_bvh_body (rayz_amd/csrc/rayz_hip.hip) packs them: two entries to a descriptor, first << 4 | type1 << 3 |
// type0 << 2 | count.  Built with g++ and run by tests/test_bvh_layouts_cpu.py and tests/test_bvh_layouts_gpu.py, which assert
// through it that every scene of tests/bvh_layout_scenes.py forms the layout it was built for.
//
//   bvh_layout_mirror scene.bin      scene.bin = u64 n_spheres, u64 n_triangles, RayzSphere[n_spheres], RayzTriangle[n_triangles]
//
// prints one JSON list, an entry per (peel, sah).
#include "../rayz_amd/csrc/bvh_build.hpp"

#include <cstdio>

int main(int argc, char** argv) {
    if (argc != 2) return std::fprintf(stderr, "usage: %s scene.bin\n", argv[0]), 2;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f) return std::fprintf(stderr, "cannot open %s\n", argv[1]), 2;
    uint64_t n[2] = {0, 0};
    if (std::fread(n, sizeof(uint64_t), 2, f) != 2 || n[0] > (1u << 24) || n[1] > (1u << 24)) return std::fprintf(stderr, "bad header\n"), 2;
    std::vector<RayzSphere> spheres(n[0]);
    std::vector<RayzTriangle> triangles(n[1]);
    if (std::fread(spheres.data(), sizeof(RayzSphere), n[0], f) != n[0] || std::fread(triangles.data(), sizeof(RayzTriangle), n[1], f) != n[1])
        return std::fprintf(stderr, "short file\n"), 2;
    std::fclose(f);
    const uint32_t ns = (uint32_t)spheres.size();
    std::printf("[");
    for (int peel = 0; peel < 2; ++peel)
        for (int sah = 0; sah < 2; ++sah) {
            const rayz_bvh::FlatBvh t = rayz_bvh::build(spheres, triangles, peel != 0, sah != 0);
            size_t inner = 0;
            for (const rayz_bvh::FlatNode& nd : t.nodes) inner += nd.count == 0;
            std::printf("%s\n{\"peel\": %d, \"sah\": %d, \"big\": [", peel || sah ? "," : "", peel, sah);
            for (size_t k = 0; k < t.big.size(); ++k) std::printf("%s%u", k ? ", " : "", t.big[k]);
            std::printf("], \"descriptors\": [");
            for (size_t k = 0; k < t.big.size(); k += 2) { // as upload_bvh_body: slots of the oversized follow the tree's
                const uint32_t first = (uint32_t)(t.order.size() + k), count = (uint32_t)std::min<size_t>(2, t.big.size() - k);
                uint32_t desc = (first << 4) | count;
                for (uint32_t j = 0; j < count; ++j)
                    if (t.big[k + j] >= ns) desc |= 1u << (2 + j);
                std::printf("%s{\"word\": %u, \"first\": %u, \"count\": %u, \"triangle\": [%u, %u]}", k ? ", " : "", desc, desc >> 4, desc & 3u,
                            (desc >> 2) & 1u, (desc >> 3) & 1u);
            }
            std::printf("], \"in_tree\": %zu, \"depth\": %u, \"budget\": %u, \"nodes\": %zu, \"inner\": %zu, \"max_big\": %zu, \"min_tree\": %zu}",
                        t.order.size(), t.depth, rayz_bvh::detail::levelsFor(t.order.size()) + rayz_bvh::detail::kSahExtraDepth, t.nodes.size(),
                        inner, rayz_bvh::kMaxBig, rayz_bvh::kMinTree);
        }
    std::printf("\n]\n");
    return 0;
}
