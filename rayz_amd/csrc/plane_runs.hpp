// Plane runs of the flat list's scan: plain C++, shared by the library (rayz_hip.hip, device layout in
// device_types.hpp, flat_scan.hpp) and the CPU test of the layout (tests/test_plane_runs.py).
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
// The scan (flat_scan.hpp: scan_blocks) tests the slots [first, end) of a section of a stream in pairs of groups, and while
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

// ---- one-radius sets of a static plane run or a speed bucket --------------------------------------
// A plane block's third field, the padded r², varies for no reason where the members' radii lie close together: such members are
// tested with ONE radius R', the largest |radius| + h among them (h = the bucket's bound on |vy − v0|, 0 in a static run), as
// a bucket's are with one speed.  Every member is then the sphere of its own centre and radius R', which contains its own at
// every time, and the set's R2 = the largest padded R'² of its members is a loop-invariant operand of the test: the blocks
// carry cx[G] cz[G] only.
constexpr size_t kRadiusSetMin = 64; // members a set needs (what a run and a bucket need, for the same costs)
constexpr uint32_t kSetGroup = 8;    // spheres of a two-field block: one 16-word scalar load
constexpr uint32_t kSetIter = 2 * kSetGroup; // slots one iteration of the set loop tests (one reject decision)

struct RadiusSet { // one record of a stream's set table (32 bytes)
    uint32_t first, end; // its slots, relative to the class's first slot: whole iterations, no pads
    uint32_t base;       // word of the stream at which the 2-field block of class slot 0 WOULD start (slot i: base + 2·i)
    float R2;            // the padded square of the set's one radius
    float cy, v0;        // its run's height, its bucket's speed (0 in a static run)
    uint32_t _pad[2];
};

struct SetPlan {
    std::vector<uint32_t> order; // the members in slot order: the sets' (by radius), then the members no set took, in their old order
    std::vector<uint32_t> count; // members of each set, a multiple of `iter`
    uint32_t setted = 0;         // members in sets = the first slot of what is left over, relative to the part's first slot
};

// The members `m` of a static run or of one speed bucket (pool indices in today's slot order; key_of(pool) = |radius| + h,
// r_of(pool) = |radius|) ordered by (key, pool index) and cut greedily: a set is closed before the member that would push
// R' − min key over min |radius| / kBucketCap, and cut down to whole iterations; fewer than kRadiusSetMin members form no set,
// and the first of them is left over (as every member of a non-finite key is).  What is left over keeps its old order.
template <class KeyOf, class ROf> SetPlan plan_sets(const std::vector<uint32_t>& m, KeyOf key_of, ROf r_of, uint32_t iter) {
    SetPlan out;
    std::vector<uint32_t> sorted;
    for (uint32_t pool : m)
        if (std::isfinite(key_of(pool))) sorted.push_back(pool);
    std::sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return key_of(a) != key_of(b) ? key_of(a) < key_of(b) : a < b; });
    size_t s = 0;
    while (s < sorted.size()) {
        const double kmin = key_of(sorted[s]);
        double rmin = r_of(sorted[s]);
        size_t e = s + 1;
        for (; e < sorted.size(); ++e) {
            const double r = std::min(rmin, (double)r_of(sorted[e]));
            if (!((double)key_of(sorted[e]) - kmin <= r / kBucketCap)) break;
            rmin = r;
        }
        const size_t n = (e - s) / iter * iter;
        if (n < kRadiusSetMin) {
            ++s;
            continue;
        }
        out.count.push_back((uint32_t)n);
        out.order.insert(out.order.end(), sorted.begin() + s, sorted.begin() + s + n);
        s += n;
    }
    out.setted = (uint32_t)out.order.size();
    std::vector<uint32_t> in_set = out.order;
    std::sort(in_set.begin(), in_set.end());
    for (uint32_t pool : m)
        if (!std::binary_search(in_set.begin(), in_set.end(), pool)) out.order.push_back(pool);
    return out;
}

// What a bucket's member of speed vy (the pool's f64 one; the buckets were cut by the f32 one) is grown by when it is tested with
// the bucket's speed v0: |vy − v0| against both, nudged up.
inline double bucket_h(double vy, float v0) {
    const double h0 = std::max(std::fabs(vy - (double)v0), std::fabs((double)(float)vy - (double)v0));
    return h0 * (1.0 + 0x1p-50) + 1e-300;
}

struct ClassSet { // one set of a class's layout (host)
    uint32_t run, first, count; // its run; its first slot, relative to the class's; its members
    int bucket;                 // its bucket, counted through the class's runs in order; -1: a static run's
    double Rp;                  // its one radius R' = max |radius| + h over its members
    float v0;                   // its bucket's speed, 0 in a static run
};
// The sets of one class: of each static run (buckets = nullptr), or of each speed bucket of each y-moving run (a y-moving run's
// remainder has none: its form carries vy).  `members` is each run's slot order and is rewritten: a run's or bucket's sets'
// members first, then what no set took, in its old order.  run_old_first / bucket_old_first: the first slot the old form still
// tests of each run (a y-moving run: its remainder's, unchanged) and of each bucket.
template <class ROf, class Vy64Of>
void plan_class_sets(const std::vector<PlaneRun>& runs, std::vector<std::vector<uint32_t>>& members, const std::vector<RunBuckets>* buckets,
                     ROf r_of, Vy64Of vy64_of, std::vector<ClassSet>& sets, std::vector<uint32_t>& run_old_first,
                     std::vector<uint32_t>& bucket_old_first) {
    sets.clear(), run_old_first.clear(), bucket_old_first.clear();
    int b = 0;
    for (size_t j = 0; j < runs.size(); ++j) {
        std::vector<uint32_t>& m = members[j];
        uint32_t at = runs[j].first, i0 = 0;
        const size_t parts = buckets ? (*buckets)[j].count.size() : 1;
        for (size_t q = 0; q < parts; ++q) {
            const uint32_t n_part = buckets ? (*buckets)[j].count[q] : (uint32_t)m.size();
            const float v0 = buckets ? (*buckets)[j].v0[q] : 0.0f;
            auto key = [&](uint32_t pool) { return (double)r_of(pool) + (buckets ? bucket_h(vy64_of(pool), v0) : 0.0); };
            const std::vector<uint32_t> part(m.begin() + i0, m.begin() + i0 + n_part);
            const SetPlan sp = plan_sets(part, key, r_of, kSetIter);
            uint32_t sat = at, k0 = 0;
            for (uint32_t n : sp.count) {
                double Rp = 0;
                for (uint32_t k = 0; k < n; ++k) Rp = std::max(Rp, key(sp.order[k0 + k]));
                sets.push_back(ClassSet{(uint32_t)j, sat, n, buckets ? b : -1, Rp, v0});
                sat += n, k0 += n;
            }
            std::copy(sp.order.begin(), sp.order.end(), m.begin() + i0);
            if (buckets) bucket_old_first.push_back(sat), ++b;
            else run_old_first.push_back(sat);
            at += n_part, i0 += n_part;
        }
        if (buckets) run_old_first.push_back(at);
    }
}

// The padded square one member of a set is held to: the member is tested as the sphere of its own centre c,
// velocity (0, v0, 0) and radius Rp >= |radius| + h, h >= |vy − v0|, and the pad rule of every scan sphere holds for it with
// r <- Rp and |v| <- |v| + h: (Rp + E)² rounded up to f32, E = 32u·(|c| + |v| + h + Rp + S), 40u for f64 rays narrowed to f32.
inline float pad_radius2_set(const double* c, const double* v, double S, double h, double Rp, bool f64_rays) {
    auto norm = [](const double* a) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); };
    const double E = (f64_rays ? 40.0 : 32.0) * 5.9604644775390625e-08 * (norm(c) + norm(v) + h + Rp + S);
    const double rp = Rp + E, sq = rp * rp;
    float f = (float)sq;
    if ((double)f < sq) f = std::nextafter(f, INFINITY);
    return f;
}
// A set's R2: the largest of these over its members, the slots [t.first, t.first + t.count) of its run (`members`: the run's slot
// order; center_of / velocity_of(pool): three doubles each).  What the set's record in the stream holds.
template <class CenterOf, class VelocityOf>
float class_set_r2(const ClassSet& t, const PlaneRun& run, const std::vector<uint32_t>& members, CenterOf center_of, VelocityOf velocity_of,
                   double S, bool f64_rays) {
    float R2 = 0.0f;
    for (uint32_t k = 0; k < t.count; ++k) {
        const uint32_t pool = members[t.first - run.first + k];
        const double h = t.bucket >= 0 ? bucket_h(velocity_of(pool)[1], t.v0) : 0.0;
        R2 = std::max(R2, pad_radius2_set(center_of(pool), velocity_of(pool), S, h, t.Rp, f64_rays));
    }
    return R2;
}

// Where a stream's set section starts: the first 64-byte boundary behind the existing content, which ends at word `end`.
// The device finds `end` from what the stream's head and bucket table already say, so neither changes.
constexpr uint32_t kSetHeader = 8; // words: {sets, copied bucket records, 0, 0, first old-form slot of each run}
constexpr uint32_t set_section(uint32_t end) { return (end + 15u) / 16u * 16u; }
static_assert(4 + kMaxPlaneRuns <= (int)kSetHeader, "the set header holds a first slot per run");

// ---- which basis the scan's reject test runs in ---------------------------------------------------
// The slots one scan tests, by the form that tests them, and the packed FMAs a sphere pair costs there under the XZ basis (e1 in
// the xz-plane) and the XY basis (e1 in the xy-plane: a plane run folds its height into K1 too).  The scan sits on its VALU-issue
// bound, so FMAs per slot price it.  XY is chosen only where it is strictly cheaper: a tie keeps the XZ kernel.
struct ScanSlots {
    uint64_t plane_static = 0, bucket = 0, plane_movy = 0, loose_static = 0, loose_movy = 0, movg = 0;
};
constexpr uint32_t kScanFormAuto = 0, kScanFormXZ = 1, kScanFormXY = 2;
// The XY basis with the one-radius sets scanned in their own two-field loop (flat_one_radius_kernel): the same basis and the same
// price order, so the layout's own choice stays XZ or XY, and a render that would scan in XY takes the sets where there are any.
constexpr uint32_t kScanFormOneRadius = 3;
// .. where the sets hold at least this many slots.  The set section costs every segment a chain of dependent scalar loads (the
// stream's head, its last bucket record, the section's header, the set records) and a loop start per set and per run or bucket that
// keeps leftovers, and the two-field loop saves little per slot.  Neither was measured by itself: from config 2's loss in the set
// kernel (1.3 % of a ≈10,000-cycle segment with ≈300 set slots) and config 3's gain (2.4 % of a ≈136,000-cycle segment with 9,872)
// the fixed cost comes to about 230 wave cycles and the saving to about a third of a cycle per slot, a break-even
// near 700 slots; the gate stands well above that estimate.
constexpr uint64_t kSetPayoffSlots = 1024;
// AUTO's gates of the primary lists (rayz_hip_scene_set_primary_lists, primary_lists.hpp): the lists are built and
// used from this many spheres and this many samples per pixel of a launch on.  Measured at 1920x1080, lists OFF -> ON, kernel ms of one launch (profiles/r15/primary_lists/README.md):
//   spheres, at 256 spp:  100: 61.8 -> 84.1 | 256: 102.1 -> 120.4 | 485: 141.1 -> 152.5 | 1,027: 241.3 -> 229.2 | 1,936: 361.0 -> 330.1
//                         | 4,097: 661.9 -> 539.2
//   spp, 10,003 spheres:  4: 37.2 -> 110.3 | 8: 65.7 -> 133.6 | 16: 115.2 -> 172.5 | 32: 211.1 -> 238.5 | 64: 400.6 -> 380.1
//   spp, 1,027 spheres:   32: 34.5 -> 40.1 | 256: 241.3 -> 229.2
// The builder's pass is a fixed cost per launch (83 ms at 10,003 spheres) that the saved camera scans repay per sample: the two
// rows put the break-even near 50 spp at 10,003 spheres and near 100 spp at 1,027, so 128 loses nowhere from 1,024 spheres on.
constexpr uint32_t kPrimaryMinSpheres = 1024;
constexpr uint32_t kPrimaryMinSpp = 128;
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
