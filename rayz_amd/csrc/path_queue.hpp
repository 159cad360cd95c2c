// path_queue.hpp — what every trace kernel shares outside its scan or walk: the per-path state (PathState), the chunk schedule's
// bounds (chunk_bounds), which pixel and chunk a queue entry is (place_item), the work queue as a wave sees it
// (WaveQueue, queue_pop) and the refill of an idle slot (path_refill).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.hpp"
#include "device_types.hpp"
#include "shade.hpp"

namespace rayz_dev {

// ---- per-path state of one of a lane's rays, and the steps every trace kernel shares ---------------------
template <class R> struct PathState {
    Pcg32 g;
    V<R> o, d, thr, acc;
    R time;
    uint32_t item, px, py, s_cur, s_end, seg;
    bool has_item, alive;
};
template <class R> __device__ __forceinline__ void path_init(PathState<R>& p) {
    p.g = Pcg32{0, 1};
    p.o = {R(0), R(0), R(0)};
    p.d = {R(0), R(0), R(1)};
    p.thr = {R(1), R(1), R(1)};
    p.acc = {R(0), R(0), R(0)};
    p.time = R(0);
    p.item = p.px = p.py = p.s_cur = p.s_end = p.seg = 0;
    p.has_item = p.alive = false;
}
// Samples of chunk k (the chunk schedule).  Every schedule starts with a run of equal chunks — all of it for a
// uniform one, all but the halving tail for the automatic one — and the host hands over that run's size and length: a lane
// that pops an item of the run computes its bounds; only the tail's few items read the table (two dependent loads in the
// refill of a pass whenever some lane pops — with 32-sample chunks that is every second pass).
template <class R> __device__ __forceinline__ void chunk_bounds(const TraceArgs<R>& A, uint32_t k, uint32_t& s0, uint32_t& s1) {
    if (k < A.chunk_n_uniform) {
        s0 = k * A.chunk_uniform;
        s1 = s0 + A.chunk_uniform;
    } else {
        s0 = A.chunk_start[k];
        s1 = A.chunk_start[k + 1];
    }
}

// ---- the work queue, as a wave sees it ------------------------------------------------------------------------
// Items come off one global counter.  A wave does not pay an atomic per refill (one word takes ≈88 atomics per µs on this
// chip: with the short items of a small scene the queue head, not the tracing, set the pace — 100 spheres ran at 3.8
// instead of 5.7 Gsamples/s at 64 spp): it reserves kQueueGrab consecutive items at a time and hands them to its lanes
// as they fall idle (ballot → prefix rank), touching the counter again only when the reserve runs out.  All fields are
// wave-uniform.  Which lane traces an item never affects the image.
// Which pixel and chunk a queue entry is: entry e = k · shard_pixels + i covers chunk k of the i-th pixel dealt.  Pixels are
// dealt in 8x8 TILES of the shard's local rows (the first A.tiled_pixels of them: whole tiles only, the rest row by row), so
// that the 64 items a wave grabs together are neighbours in both directions: their primary rays walk the same part of the
// tree (+1 … 2.6 % through the BVH, profiles/r03/tree/tile8.log).  The sums are stored by ROW-MAJOR pixel as before: `item`
// becomes k · shard_pixels + (local row · width + column), what resolve_kernel reads.  Returns k.
// (kTiled = false — the flat-list kernel, whose lanes all scan the same list: rows as they come.)
// kAdaptive (an adaptive pass, §4.14): entry e = k · n_active + j is chunk k of the j-th ACTIVE pixel; the list holds row-major
// local pixels in dealing order already, and `item` stays the compact index e.  The caller's queue guard (queue_pop: mine <
// total_items = n_active · chunks) is what keeps j inside the list.
template <class R, bool kTiled, bool kAdaptive = false>
__device__ __forceinline__ uint32_t place_item(const TraceArgs<R>& A, uint32_t& item, uint32_t& px, uint32_t& py) {
    const uint32_t per_chunk = kAdaptive ? A.n_active : A.shard_pixels;
    const uint32_t k = item / per_chunk;
    uint32_t lp = item - k * per_chunk;
    if (kAdaptive) {
        lp = A.active_list[lp];
    } else if (kTiled && lp < A.tiled_pixels) {
        const uint32_t tile = lp >> 6, w8 = A.width >> 3, trow = tile / w8, tcol = tile - trow * w8;
        lp = (trow * 8u + ((lp >> 3) & 7u)) * A.width + tcol * 8u + (lp & 7u);
        item = k * A.shard_pixels + lp;
    }
    const uint32_t lr = lp / A.width;
    px = lp - lr * A.width;
    const uint32_t tl = lr / A.tile_rows, within = lr - tl * A.tile_rows;
    py = (tl * A.shard_count + A.shard_index) * A.tile_rows + within;
    return k;
}

struct WaveQueue {
    uint32_t base = 0, count = 0; // the wave's reserve: items base .. base+count-1
    bool drained = false;         // the last reservation reached the end of the queue
};
constexpr uint32_t kQueueGrab = 64;
template <class R> __device__ __forceinline__ bool queue_empty(const WaveQueue& wq, const TraceArgs<R>& A) {
    return wq.drained && (wq.count == 0u || wq.base >= A.total_items);
}
// Every lane calls this; lanes with `need` get the next items (true + `item`) while the queue lasts.
template <class R>
__device__ __forceinline__ bool queue_pop(const TraceArgs<R>& A, WaveQueue& wq, uint32_t lane, bool need, uint32_t& item) {
    const unsigned long long need_mask = __ballot(need);
    if (need_mask == 0ull) return false;
    const uint32_t n_need = (uint32_t)__popcll(need_mask);
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(need_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)need_mask, 0u));
    unsigned long long mine;
    if (wq.count >= n_need) {
        mine = (unsigned long long)wq.base + rank;
        wq.base += n_need;
        wq.count -= n_need;
    } else { // the reserve is short: hand out what is left of it, then the head of a new reservation
        const uint32_t old_base = wq.base, old_count = wq.count, more = n_need - old_count;
        const uint32_t grab = more > A.queue_grab ? more : A.queue_grab;
        const int leader = __ffsll((long long)need_mask) - 1;
        unsigned long long nb = 0;
        if ((int)lane == leader) nb = atomicAdd(&A.counters[0], (unsigned long long)grab);
        nb = __shfl(nb, leader);
        mine = rank < old_count ? (unsigned long long)old_base + rank : nb + (rank - old_count);
        wq.base = (uint32_t)(nb + more); // (the host keeps total_items + every wave's last overshoot below 2^32)
        wq.count = grab - more;
        if (nb + grab >= (unsigned long long)A.total_items) wq.drained = true;
    }
    item = (uint32_t)mine;
    return need && mine < (unsigned long long)A.total_items;
}

// Retire a finished chunk, pop a new work item for an idle slot, start the slot's next path.
template <class R, bool kAdaptive = false>
__device__ __forceinline__ void path_refill(PathState<R>& p, const TraceArgs<R>& A, uint32_t lane, WaveQueue& wq) {
    typedef typename VecOf<R>::type r4;
    if (!p.alive && p.has_item && p.s_cur == p.s_end) {
        A.partial[p.item] = r4{p.acc.x, p.acc.y, p.acc.z, R(0)};
        p.has_item = false;
    }
    {
        uint32_t got_item = 0;
        if (queue_pop<R>(A, wq, lane, !p.alive && !p.has_item && !queue_empty<R>(wq, A), got_item)) {
            p.item = got_item;
            p.has_item = true;
            const uint32_t k = place_item<R, false, kAdaptive>(A, p.item, p.px, p.py);
            chunk_bounds<R>(A, k, p.s_cur, p.s_end);
            p.acc = {R(0), R(0), R(0)};
        }
    }
    if (!p.alive && p.has_item) { // start the next path of this slot's chunk
        const unsigned long long pixel_index = (unsigned long long)p.py * A.width + p.px;
        p.g.seed_path(A.seed, pixel_index * A.spp + p.s_cur);
        camera_ray<R>(A.cam, p.g, p.px, p.py, p.o, p.d, p.time);
        p.thr = {R(1), R(1), R(1)};
        p.seg = 0;
        p.s_cur++;
        p.alive = true;
    }
}

} // namespace rayz_dev
