"""The moments step's kernels as compiled for gfx950 (cross-compiled, as tests/test_denoise_isa.py does), from their metadata: both
instantiations exist, no register spilled, no scratch, the static LDS that DESIGN.md §6 states, at most 128 vector registers — and
names that stay out of the other kernels' counts."""
import isa_asm

TILE_LDS = 38 * 14 * 2 * 16  # the tile plus a 3-pixel halo, two 16-byte records per position: 17,024 bytes
VOTE_LDS = 256               # what the workgroup reduction behind __syncthreads_or takes


def test_temporal_moments_kernels_codegen():
    meta = isa_asm.metadata(isa_asm.device_asm())
    tm = {k: v for k, v in meta.items() if "temporal_moments_step_kernel" in k}
    assert len(tm) == 2 and sum("ILb0E" in k for k in tm) == 1 and sum("ILb1E" in k for k in tm) == 1, sorted(tm)  # moving, static
    plain = [k for k in meta if "temporal_step_kernel" in k]
    assert len(plain) == 2, plain  # the plain step's two are still there, and are not these
    for name, f in tm.items():
        assert not any(s in name for s in ("denoise_", "trace_kernel", "adaptive_pass_kernel")), name
        assert int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0, (name, f)
        assert int(f["private_segment_fixed_size"]) == 0, (name, f["private_segment_fixed_size"])  # no scratch
        assert int(f["group_segment_fixed_size"]) == TILE_LDS + VOTE_LDS, (name, f["group_segment_fixed_size"])
        assert int(f["vgpr_count"]) <= 128, (name, f["vgpr_count"])  # 4 waves per SIMD or better
        assert int(f["max_flat_workgroup_size"]) == 256, (name, f)
    for name in plain:
        assert int(meta[name]["group_segment_fixed_size"]) == 0, name  # the plain step still uses no LDS
