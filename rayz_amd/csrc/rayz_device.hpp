// rayz_device.hpp — gfx950 device code of the render path (included by rayz_hip.hip only).
//
// One work-item per pixel-sample path.  A wave keeps 64 paths in flight and re-fills finished lanes
// from a global work queue (wave64 ballot + mbcnt prefix ranks, one atomic per wave), so the sphere
// scan — ≥95 % of the time on a flat hit list — always runs with a full EXEC mask.  The scan is
// wave-uniform over the sphere index: sphere records come through the SCALAR path (s_load_dwordx4/x8
// from a constant-address-space pointer) and feed the VALU as SGPR operands, which costs no VGPRs, no
// LDS bandwidth and no 64× replicated vector loads.  Arithmetic is the "mode B" specification of
// DESIGN.md §4; every statement below has its twin in oracle/rayz_oracle.cpp namespace B, and the two
// must agree bit for bit (build with -ffp-contract=off: FMAs appear only where written).
//
// Reference semantics restated here (file:line into jlucier/rayz):
//   camera ray      src/camera.zig:59-90      sphere test   src/geom.zig:38-66
//   hit record      src/hit.zig:25-41         scatter       src/material.zig:73-160,179-211
//   textures        src/material.zig:19-51    bounce loop   src/renderer.zig:103-126 (recursion → loop)
//   pixel mean      src/renderer.zig:86-95
#pragma once

#include "device_types.hpp"          // address-space macros, vector typedefs, group sizes, DevScene, DevCamera, TraceArgs
#include "device_math.hpp"           // fm / mx / sq / .., accept_root, Bits, V, Pcg32, ListRng, uniform, random_in_unit_sphere
#include "flat_scan.hpp"             // narrow phase, reject test and its bases, triangle test, packed block forms, the scan loops
#include "shade.hpp"                 // textures, background, hit record, scatter_dir, shade, camera_ray
#include "path_queue.hpp"            // PathState, chunk_bounds, place_item, WaveQueue, queue_pop, path_refill
#include "trace_kernels_flat.hpp"    // the kernels of trace_kernel_flat.hpp's text, their argument blocks, primary_lists_kernel
#include "bvh_walk.hpp"              // BvhQuery, slab test, bvh_node_step, leaves, candidates
#include "trace_kernels_bvh.hpp"     // the kernels of trace_kernel_bvh.hpp's text, the RAYZ_EXPERIMENTS includes
#include "frame_kernels.hpp"         // resolve_kernel, accumulate_kernel, tonemap_kernel
#include "known_answers_kernel.hpp"  // kat_block_discs, kat_kernel
#include "query_kernel.hpp"          // QueryArgs, query_ray, query_store, the three query kernels, query_key
#include "footprint.hpp"             // footprint_albedo_kernel and its launch (namespace rayz_dev_footprint)
