// Plane runs of the flat list's scan: plain C++, shared by the library (rayz_hip.hip, device layout in
// rayz_device.hpp) and the CPU test of the layout (tests/test_plane_runs.py).
#pragma once
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

namespace rayz_plane {

constexpr int kMaxPlaneRuns = 4;     // plane runs per velocity class
constexpr size_t kPlaneRunMin = 64;  // members a run needs

struct PlaneRun {
    float cy;            // the run's common f32 centre height
    uint32_t first, end; // its slots, relative to the class's first slot: whole group pairs
};

inline uint32_t bits32(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    return u;
}
inline float f32of(uint32_t u) {
    float x;
    std::memcpy(&x, &u, 4);
    return x;
}

// The spheres `cls` of one velocity class (pool indices, pool order; cy_of(pool) = the f32 centre height the scan streams
// hold) grouped by cy: the largest kMaxPlaneRuns groups of at least kPlaneRunMin spheres become runs, in ascending cy, each
// padded to whole pairs of `group` slots.  A run saves one packed FMA per sphere pair and costs one FMA per ray plus at most
// 2·group − 1 pad slots and a restart of the scan's prefetch: at 64 members the pads cost at most 11 % of the run's tests
// and the restart ≈ one group pair, so below ~64 a run saves too little to pay for itself.  Non-finite heights stay loose.
// Every other sphere stays loose; pool order inside a run and among the loose spheres.  Returns the slots the runs cover.
template <class CyOf>
uint32_t plan_runs(const std::vector<uint32_t>& cls, CyOf cy_of, uint32_t group, std::vector<PlaneRun>& runs,
                   std::vector<std::vector<uint32_t>>& members, std::vector<uint32_t>& loose) {
    runs.clear(), members.clear(), loose.clear();
    std::map<uint32_t, std::vector<uint32_t>> by_cy; // bits of the f32 cy -> pool indices
    for (uint32_t pool : cls) by_cy[bits32(cy_of(pool))].push_back(pool);
    std::vector<std::pair<size_t, uint32_t>> big; // (members, bits of cy)
    for (const auto& kv : by_cy)
        if (kv.second.size() >= kPlaneRunMin && std::isfinite(f32of(kv.first))) big.push_back({kv.second.size(), kv.first});
    std::sort(big.begin(), big.end(), [](const auto& a, const auto& b) { return a.first != b.first ? a.first > b.first : a.second < b.second; });
    if (big.size() > (size_t)kMaxPlaneRuns) big.resize(kMaxPlaneRuns);
    std::vector<uint32_t> chosen;
    for (const auto& b : big) chosen.push_back(b.second);
    std::sort(chosen.begin(), chosen.end(), [](uint32_t a, uint32_t b) { return f32of(a) != f32of(b) ? f32of(a) < f32of(b) : a < b; });
    uint32_t at = 0;
    for (uint32_t cyb : chosen) {
        const std::vector<uint32_t>& m = by_cy[cyb];
        const uint32_t pair = 2 * group, end = at + (uint32_t)(m.size() + pair - 1) / pair * pair;
        runs.push_back(PlaneRun{f32of(cyb), at, end});
        members.push_back(m);
        at = end;
    }
    for (uint32_t pool : cls)
        if (std::find(chosen.begin(), chosen.end(), bits32(cy_of(pool))) == chosen.end()) loose.push_back(pool);
    return at;
}

} // namespace rayz_plane
