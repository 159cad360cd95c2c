// trace_kernels_bvh.hpp — the BVH trace kernels: the round described, the kernels compiled from the text
// trace_kernel_bvh.hpp (the product kernel and the adaptive pass), and, in a RAYZ_EXPERIMENTS build, the retired experiment kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bvh_walk.hpp"
#include "device_math.hpp"
#include "device_types.hpp"
#include "flat_scan.hpp"
#include "path_queue.hpp"
#include "shade.hpp"

namespace rayz_dev {

// ---- persistent trace kernel, BVH traversal ------------------------------------------------------
// Same work items, queue and summation tree as trace_kernel.  Traversal is per lane, so the wave's lanes want
// different code at different times; each ROUND therefore runs three convergent phases instead of one divergent
// step: (N) box steps until most lanes are parked at a leaf, (L) the parked leaves' reject tests together,
// (C) the parked sphere candidates' f64 roots together.  The nearest hit (with its tie rule) does not depend on
// the order in which hittables are examined, so this scheduling changes no result — only how much pruning the
// shrinking tbest achieves.  When too few lanes still have nodes to visit, the finished lanes are shaded and
// refilled (ray regeneration) while the others keep their query state and resume.
#ifndef RAYZ_STAT_SPILL
#define RAYZ_STAT_SPILL 0x7fffffffu // tests build with a small value to exercise the spill
#endif
#define RAYZ_TRACE_KERNEL_NAME trace_kernel_bvh
#include "trace_kernel_bvh.hpp"
#define RAYZ_TRACE_KERNEL_NAME adaptive_pass_kernel_bvh // (an adaptive pass's kernel, DESIGN.md §4.14: the same text over the active list)
#define RAYZ_TRACE_KERNEL_ADAPTIVE true
#include "trace_kernel_bvh.hpp"

// The retired experiment kernels (two paths per lane; walker / shader waves — DESIGN.md §6) live in experiments/: they need the
// walk and the kernels above, and nothing else needs them.
#ifdef RAYZ_EXPERIMENTS
#include "experiments/bvh2_kernel.hpp"
#include "experiments/bvhx_kernel.hpp"
#endif

} // namespace rayz_dev
