// trace_kernel_flat.hpp — the text of the persistent flat-list trace kernel.  trace_kernels_flat.hpp includes it once per kernel,
// lists the kernels and describes the work items and the summation tree.  No include guard.
//
// THE PROTOCOL.  An includer defines RAYZ_TRACE_KERNEL_NAME (required) and whichever of the parameters below its kernel differs
// in, then includes this file.  The text defaults what was left out and undefines every parameter at its end, so nothing is
// carried from one kernel to the next:
//   RAYZ_TRACE_KERNEL_ARGS      the argument block                                            TraceArgs<R>
//   RAYZ_TRACE_KERNEL_BASIS     the reject test's basis (RayBasis)                            kBasisXZ
//   RAYZ_TRACE_KERNEL_ADAPTIVE  work items over an adaptive pass's active list (§4.14)        false
//   RAYZ_TRACE_KERNEL_SETS      the one-radius sets in a loop of their own                    false
//   RAYZ_TRACE_KERNEL_PRIMARY   camera segments from the pixels' primary lists                false
//   RAYZ_TRACE_KERNEL_CELLS     listable segments from the slab's cells                       false
// One text and kernels of their own NAMES, not further template flags on trace_kernel: tests/test_isa_invariants.py counts the
// kernels named trace_kernel.. (six) and holds each to the product's limits, so a kernel of that name is a product kernel; the
// adaptive ones are held to the same limits by tests/test_adaptive_isa.py.  Nor a shared body FUNCTION: handing the kernel's
// argument block to it changes the product kernel's register allocation; compiled once per name, trace_kernel's ISA is what it was.
//
// THE PHASES.  An iteration of the loop refills idle slots, sets up each slot's ray (scan_begin), finds its nearest hit and shades.
// RAYZ_TRACE_KERNEL_PRIMARY: each path's CAMERA segment is resolved from its pixel's primary list (primary_lists.hpp)
// instead of a scan.  An iteration of the loop is then either a LIST phase — taken while any lane of the wave holds a fresh path
// (seg == 0) on a pixel that has a list: those lanes alone take their listed slots through narrow_eval, count the segment and
// shade; a path that ends there (sky, absorption, depth) is replaced at the top of the next iteration, the chunk retired and the
// next item popped as ever — or a SCAN phase as before, once every live lane's next segment needs the scan (a later segment,
// or the camera segment of a pixel without a list).  The refill therefore repeats, wave-cooperative, until every lane holds a
// path that needs a scan or the queue is drained; nothing else differs: same streams, same sums, same segments counter.
// RAYZ_TRACE_KERNEL_CELLS: every segment whose ray crosses the members' slab under a handful of cells (slab_cells.hpp, DESIGN.md
// §4.22) is resolved from the outliers and those cells' slots.  After scan_begin each live lane learns whether its next segment is
// SHORT (a fresh path on a pixel with a primary list, where the launch has lists: A.primary may be null; no cells; a box of at most
// kMaxCells), LONG (a walk of at most kWalkColumns columns along the stretch, where the launch walks) or SCAN.  With m live lanes and
// L = min(kListLanes, m) the wave runs a list phase for the short lanes alone if they number L, else for short and long together if
// those do, else the scan for every live lane: a list phase never runs for a few lanes while the rest wait, no lane waits longer for
// its scan than the threshold lets it, and a long walk holds up short lanes only where they could not fill a phase themselves.  The
// tie rule of accept_root is order-independent, a member sits in exactly one cell and a walk names a cell once: the same
// tbest and ibest as the scan's, bit for bit.
#ifndef RAYZ_TRACE_KERNEL_NAME
#error "define RAYZ_TRACE_KERNEL_NAME before including trace_kernel_flat.hpp"
#endif
#ifndef RAYZ_TRACE_KERNEL_ARGS
#define RAYZ_TRACE_KERNEL_ARGS TraceArgs<R>
#endif
#ifndef RAYZ_TRACE_KERNEL_BASIS
#define RAYZ_TRACE_KERNEL_BASIS kBasisXZ
#endif
#ifndef RAYZ_TRACE_KERNEL_ADAPTIVE
#define RAYZ_TRACE_KERNEL_ADAPTIVE false
#endif
#ifndef RAYZ_TRACE_KERNEL_SETS
#define RAYZ_TRACE_KERNEL_SETS false
#endif
#ifndef RAYZ_TRACE_KERNEL_PRIMARY
#define RAYZ_TRACE_KERNEL_PRIMARY false
#endif
#ifndef RAYZ_TRACE_KERNEL_CELLS
#define RAYZ_TRACE_KERNEL_CELLS false
#endif
template <class R, int NR> __global__ __launch_bounds__(256, (flat_waves<R, NR>())) void RAYZ_TRACE_KERNEL_NAME(const RAYZ_TRACE_KERNEL_ARGS A) {
    constexpr bool kAdaptive = RAYZ_TRACE_KERNEL_ADAPTIVE; // work items over the active list (place_item)
    constexpr int kBasis = RAYZ_TRACE_KERNEL_BASIS;        // the reject test's basis (RayBasis)
    constexpr bool kSets = RAYZ_TRACE_KERNEL_SETS;         // the one-radius sets in their own loop (scan_plane_class)
    constexpr bool kPrimary = RAYZ_TRACE_KERNEL_PRIMARY;   // camera segments from the pixels' primary lists
    constexpr bool kCells = RAYZ_TRACE_KERNEL_CELLS;       // listable segments from the slab's cells (and the primary lists, where launched with them)
    const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    PathState<R> p[NR];
#pragma unroll
    for (int r = 0; r < NR; ++r) path_init<R>(p[r]);
    uint32_t nseg = 0;
    WaveQueue wq; // wave-uniform
#ifdef RAYZ_FLAT_PROFILE // measurement build only: wave time per phase (refill, ray setup, scan, narrow flush, shade)
    // .. list phases (their own slot, 5); fp: wave-uniform counts of the cells kernels — 0 secondary segments, 1 listable ones, 2 segments a
    // cell lane's list phase resolved, 3 their cell entries, 4 list phases, 5 their lanes, 6 live lanes at scans, 7 walked secondary
    // segments, 8 + k listable secondary segments whose box covers k cells (k <= 12).  With -DRAYZ_FLAT_PROFILE_WALK the slots 8 .. 15
    // hold instead the histogram of the secondary segments whose box failed on its cell count alone, by the columns their walk would
    // cross (<= 4, 8, 12, 16, 24, 32, 48, more; whatever the cap): the count in the low 30 bits, the walk's cells above them.
    unsigned long long ft[6] = {0, 0, 0, 0, 0, 0}, ft0 = __builtin_amdgcn_s_memtime(), fiters = 0, fp[21] = {};
    uint32_t fcells[NR]; // per slot: 13 = not listable by the cells, 14 = walked
#ifdef RAYZ_FLAT_PROFILE_WALK
    uint32_t fbin[NR], fwalk[NR]; // per slot: the bin (8: the box did not fail on its count) and the walk's cells
    unsigned long long fhist[8] = {0, 0, 0, 0, 0, 0, 0, 0}; // per lane
#endif
#pragma unroll
    for (int r = 0; r < NR; ++r) fcells[r] = 13u;
#define RAYZ_FPROF(k) { const unsigned long long now_ = __builtin_amdgcn_s_memtime(); ft[k] += now_ - ft0; ft0 = now_; }
#else
#define RAYZ_FPROF(k)
#endif

    for (;;) {
        // ---- retire finished chunks, refill idle slots ----
        bool any = false;
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            path_refill<R, kAdaptive>(p[r], A, lane, wq);
            any = any || p[r].alive;
        }
        if (__ballot(any) == 0ull) break; // queue drained and every slot idle: the wave is done

        RAYZ_FPROF(0)
        // ---- nearest hit (full EXEC; idle tail slots recompute their last ray, results unused) ----
        ScanRay<R, kBasis> ray[NR];
        V<R> ud[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            ud[r] = unit(p[r].d);
            scan_begin<R, NR>(ray[r], p[r].o, p[r].d, ud[r], p[r].time);
        }
        RAYZ_FPROF(1)
        // ---- list phase (kPrimary): fresh paths on pixels with a list; the scan waits until the wave has none ----
        bool listed[NR];
#pragma unroll
        for (int r = 0; r < NR; ++r) listed[r] = false;
        bool list_phase = false;
        if constexpr (kPrimary) {
            uint32_t lp[NR];
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                lp[r] = 0u;
                if (p[r].alive && p[r].seg == 0u) {
                    lp[r] = p[r].item - (p[r].item / A.shard_pixels) * A.shard_pixels; // the local pixel (place_item, rows as they come)
                    listed[r] = A.primary[lp[r]] != rayz_primary::kNoList;
                }
                list_phase = list_phase || listed[r];
            }
            list_phase = __ballot(list_phase) != 0ull;
            if (list_phase) {
#pragma unroll
                for (int r = 0; r < NR; ++r)
                    if (listed[r]) { // scan_begin's tbest, ibest and inv_a2; every listed slot decided by the narrow phase
                        const uint32_t count = A.primary[lp[r]];
                        for (uint32_t j = 0; j < count; ++j) {
                            const uint32_t slot = A.primary[(size_t)(j + 1u) * A.shard_pixels + lp[r]];
                            narrow_eval<R>(A.sc.slot64[2 * slot], A.sc.slot64[2 * slot + 1], (int)A.sc.slot_pool[slot], ray[r].o, ray[r].d,
                                           ray[r].time, ray[r].inv_a2, A.tmin, ray[r].tbest, ray[r].ibest);
                        }
                    }
                RAYZ_FPROF(5)
            }
        }
        if constexpr (kCells) {
            namespace rc = rayz_cells;
            // A live lane is SHORT (a primary list, no cells, or a box of at most kMaxCells), LONG (a walk along the stretch) or SCAN.
            // The walker's state, five integers: the column at hand and the last, the minor index at hand and the column's last, and
            // `aux` — a box lane's first minor index (its columns are the box's z rows, all of one range), a walk lane's major axis.
            enum : uint32_t { kNone = 0u, kBoxLane = 1u, kWalkLane = 2u };
            uint32_t lp[NR], cls[NR], col[NR], col_last[NR], mi[NR], mi_last[NR], aux[NR];
            bool prim[NR], is_short = false, is_long = false, any_alive = false;
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                lp[r] = 0u;
                prim[r] = false;
                cls[r] = kNone;
                col[r] = col_last[r] = aux[r] = 0u;
                mi[r] = 1u, mi_last[r] = 0u; // (the first step enters the first column)
                bool shrt = false, lng = false;
#ifdef RAYZ_FLAT_PROFILE
                fcells[r] = 13u;
#ifdef RAYZ_FLAT_PROFILE_WALK
                fbin[r] = 8u, fwalk[r] = 0u;
#endif
#endif
                if (p[r].alive) {
                    if (p[r].seg == 0u && A.primary != nullptr) {
                        lp[r] = p[r].item - (p[r].item / A.shard_pixels) * A.shard_pixels;
                        prim[r] = A.primary[lp[r]] != rayz_primary::kNoList;
                    }
                    shrt = prim[r];
                    if (!prim[r]) { // f64 on the widened o and d: bit for bit the ray narrow_eval gets
                        const double ox = (double)ray[r].o.x, oy = (double)ray[r].o.y, oz = (double)ray[r].o.z;
                        const double dx = (double)ray[r].d.x, dy = (double)ray[r].d.y, dz = (double)ray[r].d.z;
                        rc::CellStretch st;
                        bool count_only;
                        const rc::CellBox box = rc::cells_stretch(A.grid, ox, oy, oz, dx, dy, dz, st, count_only);
                        if (box.kind == rc::kNoCells) shrt = true;
                        else if (box.kind == rc::kSomeCells) {
                            if (!(rc::overflowed_cells(A.grid) && rc::box_overflowed(A.grid, A.cells + rc::kTableHead, box))) {
                                shrt = true;
                                cls[r] = kBoxLane;
                                col[r] = box.j0 - 1u, col_last[r] = box.j1, aux[r] = box.i0, mi_last[r] = box.i1, mi[r] = box.i1 + 1u;
#ifdef RAYZ_FLAT_PROFILE
                                fcells[r] = (box.i1 - box.i0 + 1u) * (box.j1 - box.j0 + 1u);
#endif
                            }
                        } else if (count_only && rc::walks(A.grid)) {
                            const rc::CellWalk w = rc::cells_walk(A.grid, A.cells + rc::kTableHead, box, st, ox, oz, dx, dz);
                            if (w.kind == rc::kSomeCells) {
                                lng = true;
                                cls[r] = kWalkLane;
                                col[r] = w.k0 - 1u, col_last[r] = w.k1, aux[r] = w.xmajor;
                            }
                        }
#ifdef RAYZ_FLAT_PROFILE
                        if (box.kind == rc::kNoCells) fcells[r] = 0u;
                        if (lng) fcells[r] = 14u;
#ifdef RAYZ_FLAT_PROFILE_WALK
                        if (count_only) {
                            const bool xm = (box.kind & rc::kWalkMajorX) != 0u;
                            const uint32_t k0 = xm ? box.i0 : box.j0, k1 = xm ? box.i1 : box.j1, n = k1 - k0 + 1u;
                            fbin[r] = n <= 4u ? 0u : n <= 8u ? 1u : n <= 12u ? 2u : n <= 16u ? 3u : n <= 24u ? 4u : n <= 32u ? 5u : n <= 48u ? 6u : 7u;
                            for (uint32_t k = k0; k <= k1; ++k) {
                                uint32_t m0 = 1u, m1 = 0u;
                                if (rc::walk_column(A.grid, box, st, xm, k, ox, oz, dx, dz, m0, m1)) fwalk[r] += m1 - m0 + 1u;
                            }
                        }
#endif
#endif
                    }
                }
                if (rc::one_class(A.grid)) shrt = shrt || lng, lng = false;
                listed[r] = shrt; // (for now: the rule below may add the long lanes)
                is_short = is_short || shrt;
                is_long = is_long || lng;
                any_alive = any_alive || p[r].alive;
            }
            const uint32_t n_short = (uint32_t)__popcll(__ballot(is_short)), n_long = (uint32_t)__popcll(__ballot(is_long));
            const uint32_t n_alive = (uint32_t)__popcll(__ballot(any_alive));
            const uint32_t need = n_alive < rc::list_lanes(A.grid) ? n_alive : rc::list_lanes(A.grid);
            // lanes keep company of their own kind: the short ones alone if they suffice, else short and long together, else the scan
            const bool with_long = n_short < need; // (wave-uniform)
            const uint32_t n_listed = with_long ? n_short + n_long : n_short;
#pragma unroll
            for (int r = 0; r < NR; ++r) listed[r] = listed[r] || (with_long && cls[r] == kWalkLane);
            list_phase = n_listed != 0u && n_listed >= need;
            // (the hint: most iterations are list phases; it also keeps the scan loops laid out in the order of the kernels these were
            // made from, which tests/test_slab_cells_isa.py compares loop by loop)
            if (__builtin_expect(list_phase, 1)) {
#pragma unroll
                for (int r = 0; r < NR; ++r) {
                    // round one: a primary lane's listed slots, a cell lane's outliers (the head of the table): an indexed list either way
                    const uint32_t* src = A.cells;
                    uint32_t stride = 1u, count = 0u;
                    if (listed[r]) {
                        count = A.grid.n_outliers;
                        if (prim[r]) src = A.primary + (size_t)A.shard_pixels + lp[r], stride = A.shard_pixels, count = A.primary[lp[r]];
                    }
                    for (uint32_t k = 0; __ballot(k < count) != 0ull; ++k)
                        if (k < count) {
                            const uint32_t slot = src[(size_t)k * stride];
                            narrow_eval<R>(A.sc.slot64[2 * slot], A.sc.slot64[2 * slot + 1], (int)A.sc.slot_pool[slot], ray[r].o, ray[r].d,
                                           ray[r].time, ray[r].inv_a2, A.tmin, ray[r].tbest, ray[r].ibest);
                        }
                    // round two: one walker for box and walk lanes, one entry per step whatever cell it comes from
                    bool walking = listed[r] && cls[r] != kNone;
                    uint32_t e = 0u;
                    uint4 rec{0u, 0u, 0u, 0u}; // the cell at hand: its count and kCellCap slots
                    static_assert(rc::kCellWords == 4u, "a cell's record is one 16-byte load");
                    for (;;) {
                        while (walking && e >= rec.x) { // on to the next cell that holds an entry (no listed lane's cells hold an overflowed one)
                            bool have = true;
                            if (++mi[r] > mi_last[r]) { // on to the next column
                                if (++col[r] > col_last[r]) walking = false, have = false;
                                else if (cls[r] == kBoxLane) mi[r] = aux[r];
                                else { // a walk lane: the column's range from the widened ray again (nothing f64 is held across narrow_eval)
                                    const double ox = (double)ray[r].o.x, oz = (double)ray[r].o.z, dx = (double)ray[r].d.x, dz = (double)ray[r].d.z;
                                    rc::CellStretch st;
                                    bool count_only;
                                    const rc::CellBox box = rc::cells_stretch(A.grid, ox, (double)ray[r].o.y, oz, dx, (double)ray[r].d.y, dz, st, count_only);
                                    uint32_t m0 = 1u, m1 = 0u;
                                    have = rc::walk_column(A.grid, box, st, aux[r] != 0u, col[r], ox, oz, dx, dz, m0, m1);
                                    mi[r] = have ? m0 : 1u, mi_last[r] = have ? m1 : 0u;
                                }
                            }
                            e = 0u, rec.x = 0u;
                            if (have) {
                                const uint32_t at = cls[r] == kWalkLane && aux[r] != 0u ? mi[r] * A.grid.nx + col[r] : col[r] * A.grid.nx + mi[r];
                                rec = *(const uint4*)(A.cells + rc::kTableHead + (size_t)at * rc::kCellWords);
                            }
                        }
                        if (__ballot(walking) == 0ull) break;
                        if (walking) {
                            const uint32_t slot = e == 0u ? rec.y : e == 1u ? rec.z : rec.w;
                            ++e;
                            narrow_eval<R>(A.sc.slot64[2 * slot], A.sc.slot64[2 * slot + 1], (int)A.sc.slot_pool[slot], ray[r].o, ray[r].d,
                                           ray[r].time, ray[r].inv_a2, A.tmin, ray[r].tbest, ray[r].ibest);
                        }
#ifdef RAYZ_FLAT_PROFILE
                        fp[3] += (unsigned long long)__popcll(__ballot(walking));
#endif
                    }
#ifdef RAYZ_FLAT_PROFILE
                    fp[2] += (unsigned long long)__popcll(__ballot(listed[r] && !prim[r]));
#endif
                }
#ifdef RAYZ_FLAT_PROFILE
                fp[4]++;
                fp[5] += n_listed;
#endif
                RAYZ_FPROF(5)
            }
#ifdef RAYZ_FLAT_PROFILE
            else fp[6] += n_alive;
#endif
        }
        if (!list_phase) {
#ifdef RAYZ_FLAT_PROFILE
            fiters++;
            scan_sphere_classes<R, NR, kSets>(A.sc, ray, A.tmin);
            RAYZ_FPROF(2)
            narrow_flush<R, NR>(A.sc, ray, A.tmin);
            scan_triangles<R, NR>(A.sc, ray, A.tmin);
            RAYZ_FPROF(3)
#else
            scan_spheres<R, NR, kSets>(A.sc, ray, A.tmin);
#endif
        }

        // ---- shade ----
#ifdef RAYZ_FLAT_PROFILE
        if constexpr (kCells) { // (the ballots in front of the divergent shading: every lane keeps the same counts)
#pragma unroll
            for (int r = 0; r < NR; ++r) {
                const bool secondary = p[r].alive && (!list_phase || listed[r]) && p[r].seg != 0u;
                fp[0] += (unsigned long long)__popcll(__ballot(secondary));
                fp[1] += (unsigned long long)__popcll(__ballot(secondary && fcells[r] <= 12u));
                fp[7] += (unsigned long long)__popcll(__ballot(secondary && fcells[r] == 14u));
#ifdef RAYZ_FLAT_PROFILE_WALK
                if (secondary && fbin[r] < 8u)
                    for (uint32_t k = 0; k < 8u; ++k) fhist[k] += fbin[r] == k ? 1ull + ((unsigned long long)fwalk[r] << 30) : 0ull;
#else
                for (uint32_t k = 0; k <= 12u; ++k) fp[8 + k] += (unsigned long long)__popcll(__ballot(secondary && fcells[r] == k));
#endif
            }
        }
#endif
#pragma unroll
        for (int r = 0; r < NR; ++r)
            if (p[r].alive && (!list_phase || listed[r])) {
                nseg++;
                p[r].seg++;
                bool cont = shade<R>(A.sc, p[r].g, p[r].o, p[r].d, ud[r], p[r].time, ray[r].tbest, ray[r].ibest, p[r].thr,
                                     p[r].acc);
                if (p[r].seg >= A.max_bounces) cont = false; // depth exhausted → black, src/renderer.zig:104-105
                p[r].alive = cont;
            }
        RAYZ_FPROF(4)
    }
#ifdef RAYZ_FLAT_PROFILE
#ifdef RAYZ_FLAT_PROFILE_WALK
    for (int k = 0; k < 8; ++k) {
        for (int off = 32; off > 0; off >>= 1) fhist[k] += __shfl_xor(fhist[k], off);
        fp[8 + k] = fhist[k];
    }
#endif
    if (lane == 0) {
        for (int k = 0; k < 5; ++k) atomicAdd(&A.counters[4 + k], ft[k]);
        atomicAdd(&A.counters[9], fiters);
        atomicAdd(&A.counters[10], ft[5]);
        for (int k = 0; k < 21; ++k) atomicAdd(&A.counters[11 + k], fp[k]);
    }
#endif
    // ---- counters: one atomic per wave ----
    unsigned long long tot = nseg;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) tot += __shfl_xor(tot, off);
    if (lane == 0) atomicAdd(&A.counters[1], tot);
}
#undef RAYZ_TRACE_KERNEL_NAME
#undef RAYZ_TRACE_KERNEL_ARGS
#undef RAYZ_TRACE_KERNEL_BASIS
#undef RAYZ_TRACE_KERNEL_ADAPTIVE
#undef RAYZ_TRACE_KERNEL_SETS
#undef RAYZ_TRACE_KERNEL_PRIMARY
#undef RAYZ_TRACE_KERNEL_CELLS
