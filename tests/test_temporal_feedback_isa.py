"""The feedback mode's kernels as compiled for gfx950 (cross-compiled, as tests/test_temporal_moments_isa.py does), from their
metadata: both instantiations of the step exist, no register spilled, no scratch, the moments step's static LDS, at most 128
vector registers, a workgroup of 256; the write kernel uses no LDS and no scratch."""
import isa_asm

TILE_LDS = 38 * 14 * 2 * 16  # the tile plus a 3-pixel halo, two 16-byte records per position: 17,024 bytes
VOTE_LDS = 256               # what the workgroup reduction behind __syncthreads_or takes


def test_temporal_feedback_kernels_codegen():
    meta = isa_asm.metadata(isa_asm.device_asm())
    step = {k: v for k, v in meta.items() if "temporal_feedback_step_kernel" in k}
    assert len(step) == 2 and sum("ILb0E" in k for k in step) == 1 and sum("ILb1E" in k for k in step) == 1, sorted(step)  # moving, static
    for name, f in step.items():
        assert not any(s in name for s in ("denoise_", "trace_kernel", "adaptive_pass_kernel", "temporal_moments_step_kernel",
                                           "temporal_step_kernel")), name
        assert int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0, (name, f)
        assert int(f["private_segment_fixed_size"]) == 0, (name, f["private_segment_fixed_size"])  # no scratch
        assert int(f["group_segment_fixed_size"]) == TILE_LDS + VOTE_LDS, (name, f["group_segment_fixed_size"])
        assert int(f["vgpr_count"]) <= 128, (name, f["vgpr_count"])  # 4 waves per SIMD or better
        assert int(f["max_flat_workgroup_size"]) == 256, (name, f)
    write = {k: v for k, v in meta.items() if "temporal_feedback_write_kernel" in k}
    assert len(write) == 1, sorted(write)
    for name, f in write.items():
        assert int(f["group_segment_fixed_size"]) == 0 and int(f["private_segment_fixed_size"]) == 0, (name, f)
        assert int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0, (name, f)
        assert int(f["max_flat_workgroup_size"]) == 256, (name, f)
