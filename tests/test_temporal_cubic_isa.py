"""The cubic resampling mode's two kernels as compiled for gfx950 (cross-compiled, as tests/test_temporal_moments_isa.py does), from
their metadata: each exists once, no register spilled, no scratch, at most 128 vector registers; the plain one uses no LDS, the
moments one the moments kernel's 17,280 bytes — and their names stay out of the other temporal kernels' counts."""
import isa_asm

MOMENTS_LDS = 38 * 14 * 2 * 16 + 256  # the moments kernel's staged tile and its vote (tests/test_temporal_moments_isa.py)


def test_temporal_cubic_kernels_codegen():
    meta = isa_asm.metadata(isa_asm.device_asm())
    plain = {k: v for k, v in meta.items() if "temporal_cubic_step_kernel" in k}
    moments = {k: v for k, v in meta.items() if "temporal_cubic_moments_step_kernel" in k}
    assert len(plain) == 1 and len(moments) == 1, (sorted(plain), sorted(moments))
    for name, f in {**plain, **moments}.items():
        assert int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0, (name, f)
        assert int(f["private_segment_fixed_size"]) == 0, (name, f["private_segment_fixed_size"])  # no scratch
        assert int(f["vgpr_count"]) <= 128, (name, f["vgpr_count"])  # 4 waves per SIMD or better
        assert int(f["max_flat_workgroup_size"]) == 256, (name, f)
    assert int(next(iter(plain.values()))["group_segment_fixed_size"]) == 0
    assert int(next(iter(moments.values()))["group_segment_fixed_size"]) == MOMENTS_LDS == 17280
    # the existing kernels' counts by substring are what they were
    for stem, n in (("temporal_step_kernel", 2), ("temporal_moments_step_kernel", 2), ("temporal_feedback_step_kernel", 2)):
        assert sum(stem in k for k in meta) == n, (stem, [k for k in meta if stem in k])
