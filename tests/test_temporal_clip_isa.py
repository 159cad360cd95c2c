"""The clip mode's kernels as compiled for gfx950 (cross-compiled, as tests/test_temporal_background_isa.py does), from their
metadata: exactly four, in a namespace of their own — the moving plain and the moving moments step, each with and without background
history —, no register spilled, no scratch, at most 128 vector registers, workgroups of 256, and the moments step's LDS in all
four: the plain clip kernel stages the same tile — and names that stay out of the other kernels' counts."""
import isa_asm

TILE_LDS = 38 * 14 * 2 * 16  # the tile plus a 3-pixel halo, two 16-byte records per position: 17,024 bytes
VOTE_LDS = 256               # what the workgroup reduction behind __syncthreads_or takes
KINDS = ("clip_plain_kernel", "clip_moments_kernel")
OTHERS = ("denoise_", "trace_kernel", "adaptive_pass_kernel", "temporal_step_kernel", "temporal_moments_step_kernel",
          "temporal_feedback_step_kernel", "temporal_counts_kernel", "temporal_counts_moments_kernel", "temporal_cubic_", "temporal_bg_",
          "cells_", "primary_", "sparse_", "upscale_", "footprint_")


def test_temporal_clip_kernels_codegen():
    meta = isa_asm.metadata(isa_asm.device_asm())
    mine = {k: v for k, v in meta.items() if "rayz_dev_clip" in k.split("ILb")[0]}
    assert len(mine) == 4, sorted(mine)
    for kind in KINDS:
        group = [k for k in mine if f"{len(kind)}{kind}ILb" in k]  # (the mangled name: its length, then the name)
        assert len(group) == 2 and sum("ILb0E" in k for k in group) == 1 and sum("ILb1E" in k for k in group) == 1, (kind, sorted(mine))
    for name, f in mine.items():
        assert name.startswith("_ZN13rayz_dev_clip"), name
        assert not any(s in name for s in OTHERS), name
        print(name, "vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"], "lds", f["group_segment_fixed_size"])
        assert int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0, (name, f)
        assert int(f["private_segment_fixed_size"]) == 0, (name, f["private_segment_fixed_size"])  # no scratch
        assert int(f["vgpr_count"]) <= 128, (name, f["vgpr_count"])  # 4 waves per SIMD or better
        assert int(f["max_flat_workgroup_size"]) == 256, (name, f)
        assert int(f["group_segment_fixed_size"]) == TILE_LDS + VOTE_LDS, (name, f["group_segment_fixed_size"])
