// trace_kernels_flat.hpp — the flat-list trace kernels: the list of kernels compiled from the text trace_kernel_flat.hpp (the
// product kernel, its other basis, the one-radius sets, the adaptive pass, and the three scan forms over primary lists and over
// the slab's cells), their argument blocks, and the primary lists' builder.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.hpp"
#include "device_types.hpp"
#include "flat_scan.hpp"
#include "path_queue.hpp"
#include "primary_lists.hpp"
#include "shade.hpp"
#include "slab_cells.hpp"

namespace rayz_dev {

// ---- the persistent trace kernel (flat hit list) ----------------------------------------------------------
// Work item = (pixel of this shard, chunk k of the pixel's chunk schedule: samples chunk_start[k] .. chunk_start[k+1]).
// The schedule puts the big chunks first and ends in small ones (host: chunk_schedule), so the queue's tail is made
// of short items.  Items are numbered chunk-major so
// that the 64 lanes of a wave start on 64 neighbouring pixels.  Each of a lane's NR slots owns one item at a
// time, runs its paths one after the other, adds their radiance in sample order, and stores the chunk sum to
// partial[item]; resolve_kernel adds the chunk sums of a pixel in chunk order.  The summation tree is therefore
// fixed by the chunk schedule alone — a function of (width, height, spp, chunk_spp) — not by the launch, the grid
// size, NR or the number of GPUs.
#ifndef RAYZ_FLAT_WAVES_F64
#define RAYZ_FLAT_WAVES_F64 4
#endif
template <class R, int NR> constexpr int flat_waves() { return sizeof(R) == 8 ? RAYZ_FLAT_WAVES_F64 : NR == 1 ? 4 : 3; }
// Every kernel below is trace_kernel_flat.hpp once more: its own complete set of the text's parameters, then the include (the text
// defaults what is left out and undefines all of them at its end).
#define RAYZ_TRACE_KERNEL_NAME trace_kernel
#include "trace_kernel_flat.hpp"
// The same text once more with the xy basis (kBasisXY: 5 packed FMAs per sphere pair in plane runs and buckets, 9 on a loose
// y-moving sphere): the host launches it for the scenes whose scan it prices lower (rayz_plane::scan_price).  A kernel of its
// own name, so that trace_kernel's code is what it was.
#define RAYZ_TRACE_KERNEL_NAME flat_xy_kernel
#define RAYZ_TRACE_KERNEL_BASIS kBasisXY
#include "trace_kernel_flat.hpp"
// The xy basis with the one-radius sets scanned by scan_sets (scan_plane_class's kSets), for scenes that
// have such sets.  A kernel of its own name for the reasons flat_xy_kernel is one (tests/test_one_radius_isa.py holds it to the limits).
#define RAYZ_TRACE_KERNEL_NAME flat_one_radius_kernel
#define RAYZ_TRACE_KERNEL_BASIS kBasisXY
#define RAYZ_TRACE_KERNEL_SETS true
#include "trace_kernel_flat.hpp"
#define RAYZ_TRACE_KERNEL_NAME adaptive_pass_kernel // (an adaptive pass's kernel, DESIGN.md §4.14: the same text over the active list)
#define RAYZ_TRACE_KERNEL_ADAPTIVE true
#include "trace_kernel_flat.hpp"
// The three scan forms once more with the camera segments resolved from the pixels' primary lists: kernels
// of their own names, which the ISA tests of the kernels above do not count (tests/test_primary_lists_isa.py holds these).
// Their argument block is the trace kernels' with the lists behind it (a block of its own: a field more in TraceArgs changes
// every other kernel's code object).
template <class R> struct PrimaryTraceArgs : TraceArgs<R> {
    const uint32_t* primary; // the shard's primary lists, word j of local pixel i at [j · shard_pixels + i]
};
#define RAYZ_TRACE_KERNEL_NAME primary_xz_kernel
#define RAYZ_TRACE_KERNEL_ARGS PrimaryTraceArgs<R>
#define RAYZ_TRACE_KERNEL_PRIMARY true
#include "trace_kernel_flat.hpp"
#define RAYZ_TRACE_KERNEL_NAME primary_xy_kernel
#define RAYZ_TRACE_KERNEL_ARGS PrimaryTraceArgs<R>
#define RAYZ_TRACE_KERNEL_PRIMARY true
#define RAYZ_TRACE_KERNEL_BASIS kBasisXY
#include "trace_kernel_flat.hpp"
#define RAYZ_TRACE_KERNEL_NAME primary_one_radius_kernel
#define RAYZ_TRACE_KERNEL_ARGS PrimaryTraceArgs<R>
#define RAYZ_TRACE_KERNEL_PRIMARY true
#define RAYZ_TRACE_KERNEL_BASIS kBasisXY
#define RAYZ_TRACE_KERNEL_SETS true
#include "trace_kernel_flat.hpp"
// The three scan forms a third time with every listable segment resolved from the slab's cells (slab_cells.hpp, DESIGN.md
// §4.22), and a fresh path's from its pixel's primary list where the launch has lists (`primary` may be null): kernels of their own
// names again, and in a namespace of their own, rayz_dev_cells: tests/test_sparse_isa.py takes every kernel of rayz_dev it has no record
// of for a sparse-render kernel (tests/test_slab_cells_isa.py holds these).  Their argument block is the primary kernels' with the grid
// and the table behind it.
template <class R> struct CellsTraceArgs : PrimaryTraceArgs<R> {
    rayz_cells::CellGrid grid;
    const uint32_t* cells; // [kTableHead outlier slots][grid.nx · grid.nz records of kCellWords], 16-byte aligned
};
} // namespace rayz_dev (reopened below)
namespace rayz_dev_cells {
using namespace rayz_dev;
#define RAYZ_TRACE_KERNEL_NAME cells_xz_kernel
#define RAYZ_TRACE_KERNEL_ARGS CellsTraceArgs<R>
#define RAYZ_TRACE_KERNEL_CELLS true
#include "trace_kernel_flat.hpp"
#define RAYZ_TRACE_KERNEL_NAME cells_xy_kernel
#define RAYZ_TRACE_KERNEL_ARGS CellsTraceArgs<R>
#define RAYZ_TRACE_KERNEL_CELLS true
#define RAYZ_TRACE_KERNEL_BASIS kBasisXY
#include "trace_kernel_flat.hpp"
#define RAYZ_TRACE_KERNEL_NAME cells_one_radius_kernel
#define RAYZ_TRACE_KERNEL_ARGS CellsTraceArgs<R>
#define RAYZ_TRACE_KERNEL_CELLS true
#define RAYZ_TRACE_KERNEL_BASIS kBasisXY
#define RAYZ_TRACE_KERNEL_SETS true
#include "trace_kernel_flat.hpp"
} // namespace rayz_dev_cells
namespace rayz_dev {

// ---- the primary lists' builder -----------------------------------------------------------------------------
// One lane per local pixel of the shard (place_item's numbering, rows as they come): every sphere of the pool, by its slot, through
// rayz_primary::beam_may_hit in f64; the slots that pass are the pixel's list, kNoList its count when more than kListK do.  The
// loop is wave-uniform (the sphere's record arrives through scalar loads); `real_slots` names the slots that hold a sphere, in
// slot order: a pad's record is no sphere and may never become a candidate.
struct PrimaryArgs {
    rayz_primary::BeamCamera cam;
    const d4* slot64;
    const uint32_t* real_slots;
    uint32_t* lists; // [(kListK + 1) · shard_pixels]
    uint32_t n_real, width, tile_rows, shard_index, shard_count, shard_pixels;
};
__global__ __launch_bounds__(256) void primary_lists_kernel(const PrimaryArgs A) {
    const uint32_t lane_px = blockIdx.x * 256u + threadIdx.x;
    const bool live = lane_px < A.shard_pixels;
    const uint32_t lp = live ? lane_px : A.shard_pixels - 1u; // (the last block's spare lanes repeat the last pixel and store nothing)
    const uint32_t lr = lp / A.width, px = lp - lr * A.width;
    const uint32_t tl = lr / A.tile_rows, within = lr - tl * A.tile_rows;
    const uint32_t py = (tl * A.shard_count + A.shard_index) * A.tile_rows + within;
    const rayz_primary::PixelBeam beam = rayz_primary::pixel_beam(A.cam, px, py);
    uint32_t n = 0;
    for (uint32_t i = 0; i < A.n_real; ++i) {
        const uint32_t slot = A.real_slots[i];
        const d4 c4 = A.slot64[2 * slot], v4 = A.slot64[2 * slot + 1];
        const double c[3] = {c4.x, c4.y, c4.z}, v[3] = {v4.x, v4.y, v4.z};
        if (rayz_primary::beam_may_hit(beam, c, v, __builtin_sqrt(c4.w))) {
            if (live && n < rayz_primary::kListK) A.lists[(size_t)(n + 1u) * A.shard_pixels + lp] = slot;
            ++n;
        }
    }
    if (live) A.lists[lp] = n <= rayz_primary::kListK ? n : rayz_primary::kNoList;
}

} // namespace rayz_dev
