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

// ---- how far a scan reads ----------------------------------------------------------------------------------------------
// The scan (rayz_device.hpp: scan_blocks) tests the slots [first, end) of a section of a stream in pairs of groups, and while
// it tests a group it loads the next one: the furthest group it loads is the ONE behind its last pair (the loop before round 7
// loaded two).  Every section (plane blocks, loose blocks, bucket blocks, the mov-G stream) ends in kScanSpareGroups groups of
// never-hit pads, so a scan that ends with its section stays inside it.  scan_reach = one past the last slot a scan loads; the
// host holds every scan it lays out to scan_reach <= the section's slots (rayz_hip.hip: upload_body).
constexpr uint32_t kScanSpareGroups = 2;
inline uint32_t scan_reach(uint32_t first, uint32_t end, uint32_t group) {
    const uint32_t pair = 2 * group, n = end > first ? end - first : 0;
    return first + (n + pair - 1) / pair * pair + group;
}

// ---- speed buckets of a y-moving plane run -------------------------------------------------------
// A y-moving run's reject test differs from the static plane form by one stage, p2 += vy·(time·e2y), which exists only because
// vy differs from sphere to sphere.  Members of nearly one speed are tested with ONE speed v0 instead, hoisted into the ray's
// K2 like the run's height; what that leaves out, (vy − v0)·time·e2y, is at most h = |vy − v0| (|time·e2y| ≤ 1), and the host
// adds h to the radius the filter holds.  A bucket then runs the static plane form: 6 packed FMAs per sphere pair, not 7.
constexpr size_t kBucketMin = 64; // members a bucket needs (what a run needs, for the same costs)
constexpr int kBucketCap = 16;    // h ≤ r_min / 16 in a bucket: the filter's disc grows by at most (1 + 1/16)² in area

struct SpeedBucket { // one record of the stream's bucket table (32 bytes)
    float v0;            // the bucket's speed: the midpoint of its members' f32 vy
    float cy;            // its run's height
    uint32_t first, end; // its slots, relative to the class's first slot: whole group pairs, no pads
    uint32_t base;       // word of the stream at which the 3-field block of class slot 0 WOULD start (slot i: base + 3·i)
    uint32_t run;        // its run
    uint32_t _pad[2];
};

struct RunBuckets {
    std::vector<uint32_t> order;     // the run's members in slot order: the buckets' (by run, then speed), then the remainder's
    std::vector<uint32_t> count;     // members of each bucket, a multiple of 2·group
    std::vector<float> v0;           // speed of each bucket
    uint32_t bucketed = 0;           // members in buckets = the remainder's first slot, relative to the run's
};

inline float bucket_mid(float lo, float hi) { return (float)(((double)lo + (double)hi) * 0.5); }
// max |vy − v0| over [lo, hi] in f32, not rounded down
inline float bucket_half_width(float lo, float hi) {
    const double v0 = bucket_mid(lo, hi), h = std::max(v0 - (double)lo, (double)hi - v0);
    float f = (float)h;
    if ((double)f < h) f = std::nextafter(f, INFINITY);
    return f;
}

// The members `m` of one y-moving run (pool indices, pool order; vy_of(pool) = the f32 speed the scan streams hold, r_of(pool)
// = |radius|) ordered by (vy, pool index) and cut greedily into buckets: a bucket is closed before the sphere that would push
// its half width over min |radius| / kBucketCap, and cut down to whole group pairs; fewer than kBucketMin members form no
// bucket, and the first of them joins the remainder (as every sphere of a non-finite speed does).  The remainder keeps pool
// order and the run's own 4-field blocks.
template <class VyOf, class ROf> RunBuckets plan_buckets(const std::vector<uint32_t>& m, VyOf vy_of, ROf r_of, uint32_t group) {
    RunBuckets out;
    std::vector<uint32_t> sorted, rest;
    for (uint32_t pool : m) (std::isfinite(vy_of(pool)) ? sorted : rest).push_back(pool);
    std::sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return vy_of(a) != vy_of(b) ? vy_of(a) < vy_of(b) : a < b; });
    const size_t pair = 2 * (size_t)group;
    size_t s = 0;
    while (s < sorted.size()) {
        const float lo = vy_of(sorted[s]);
        double rmin = r_of(sorted[s]);
        size_t e = s + 1;
        for (; e < sorted.size(); ++e) {
            const double r = std::min(rmin, (double)r_of(sorted[e]));
            if (!((double)bucket_half_width(lo, vy_of(sorted[e])) <= r / kBucketCap)) break;
            rmin = r;
        }
        const size_t n = (e - s) / pair * pair;
        if (n < kBucketMin) {
            rest.push_back(sorted[s++]);
            continue;
        }
        out.count.push_back((uint32_t)n);
        out.v0.push_back(bucket_mid(lo, vy_of(sorted[s + n - 1])));
        out.order.insert(out.order.end(), sorted.begin() + s, sorted.begin() + s + n);
        s += n;
    }
    out.bucketed = (uint32_t)out.order.size();
    std::sort(rest.begin(), rest.end());
    out.order.insert(out.order.end(), rest.begin(), rest.end());
    return out;
}

// ---- which basis the scan's reject test runs in ---------------------------------------------------
// The slots one scan tests, by the form that tests them, and the packed FMAs a sphere pair costs there under the XZ basis (e1 in
// the xz-plane) and the XY basis (e1 in the xy-plane: a plane run folds its height into K1 too).  The scan sits on its VALU-issue
// bound, so FMAs per slot price it.  XY is chosen only where it is strictly cheaper: a tie keeps the XZ kernel.
struct ScanSlots {
    uint64_t plane_static = 0, bucket = 0, plane_movy = 0, loose_static = 0, loose_movy = 0, movg = 0;
};
constexpr uint32_t kScanFormAuto = 0, kScanFormXZ = 1, kScanFormXY = 2;
inline uint64_t scan_price(const ScanSlots& n, uint32_t form) {
    const bool xy = form == kScanFormXY;
    return (xy ? 5 : 6) * (n.plane_static + n.bucket) + 7 * (n.plane_movy + n.loose_static) + (xy ? 9 : 8) * n.loose_movy + 12 * n.movg;
}
inline uint32_t cheaper_scan_form(const ScanSlots& n) { return scan_price(n, kScanFormXY) < scan_price(n, kScanFormXZ) ? kScanFormXY : kScanFormXZ; }
// The slots of a layout: plane_slots[c] and class_slots[c] of the static (0) and mov-Y (1) classes (class_slots: runs and the
// loose spheres' whole group pairs), the mov-Y runs' buckets, the mov-G class's slots.
inline ScanSlots scan_slots(const uint32_t (&plane_slots)[2], const uint32_t (&class_slots)[2], const std::vector<RunBuckets>& buckets,
                            uint32_t movg_slots) {
    ScanSlots n;
    for (const RunBuckets& b : buckets) n.bucket += b.bucketed;
    n.plane_static = plane_slots[0], n.plane_movy = plane_slots[1] - n.bucket;
    n.loose_static = class_slots[0] - plane_slots[0], n.loose_movy = class_slots[1] - plane_slots[1];
    n.movg = movg_slots;
    return n;
}

} // namespace rayz_plane
