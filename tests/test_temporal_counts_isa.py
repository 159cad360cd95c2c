"""The counts step's kernels as compiled for gfx950 (cross-compiled, as tests/test_temporal_moments_isa.py does), from their
metadata: exactly four, in a namespace of their own, no register spilled, no scratch, at most 128 vector registers, no LDS for the
plain pair and the moments step's LDS for the moments pair — and names that stay out of the other kernels' counts."""
import isa_asm

TILE_LDS = 38 * 14 * 2 * 16  # the tile plus a 3-pixel halo, two 16-byte records per position: 17,024 bytes
VOTE_LDS = 256               # what the workgroup reduction behind __syncthreads_or takes


def test_temporal_counts_kernels_codegen():
    meta = isa_asm.metadata(isa_asm.device_asm())
    mine = {k: v for k, v in meta.items() if "rayz_dev_counts" in k.split("ILb")[0]}
    plain = {k: v for k, v in mine.items() if "temporal_counts_kernel" in k}
    moments = {k: v for k, v in mine.items() if "temporal_counts_moments_kernel" in k}
    assert len(mine) == 4 and len(plain) == 2 and len(moments) == 2, sorted(mine)
    for group in (plain, moments):
        assert sum("ILb0E" in k for k in group) == 1 and sum("ILb1E" in k for k in group) == 1, sorted(group)  # moving, static
    for name, f in mine.items():
        assert name.startswith("_ZN15rayz_dev_counts"), name
        assert not any(s in name for s in ("denoise_", "trace_kernel", "adaptive_pass_kernel", "temporal_step_kernel", "temporal_moments_step_kernel",
                                           "temporal_feedback_", "cells_", "primary_", "sparse_", "upscale_")), name
        print(name, "vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"], "lds", f["group_segment_fixed_size"])
        assert int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0, (name, f)
        assert int(f["private_segment_fixed_size"]) == 0, (name, f["private_segment_fixed_size"])  # no scratch
        assert int(f["vgpr_count"]) <= 128, (name, f["vgpr_count"])  # 4 waves per SIMD or better
        assert int(f["max_flat_workgroup_size"]) == 256, (name, f)
        assert int(f["group_segment_fixed_size"]) == (0 if name in plain else TILE_LDS + VOTE_LDS), (name, f["group_segment_fixed_size"])
