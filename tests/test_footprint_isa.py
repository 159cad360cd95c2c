"""The footprint-albedo kernel as compiled for gfx950 (cross-compiled, as tests/test_denoise_isa.py does), from the kernels' metadata
alone: one instantiation per factor with and without the count, none of which spills a register or uses scratch; it lives in a
namespace of its own, and its names stay out of every count the other ISA tests make by substring."""
import isa_asm

KEPT_OUT = ("query", "chain", "trace_kernel", "denoise_", "primary_", "cells_", "flat_xy_kernel", "flat_one_radius_kernel",
            "adaptive_pass_kernel", "temporal_", "rayz_dev_counts")


def test_footprint_kernel_codegen():
    meta = isa_asm.metadata(isa_asm.device_asm())
    fp = {k: v for k, v in meta.items() if "footprint_albedo_kernel" in k}
    assert len(fp) == 3 * 2, sorted(fp)  # f = 2, 3, 4 x {albedo, albedo and count}
    for name, f in fp.items():
        assert name.startswith("_ZN18rayz_dev_footprint23footprint_albedo_kernelILi"), name  # not in rayz_dev (_ZN8rayz_dev..)
        assert not any(word in name for word in KEPT_OUT), name
        print(name, "vgpr", f["vgpr_count"], "sgpr", f["sgpr_count"])
        assert int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0, (name, f)
        assert int(f["private_segment_fixed_size"]) == 0, (name, f["private_segment_fixed_size"])  # no scratch
        assert int(f["group_segment_fixed_size"]) == 0, (name, f["group_segment_fixed_size"])  # no LDS
    assert sorted(k[len("_ZN18rayz_dev_footprint23footprint_albedo_kernelILi"):][:5] for k in fp) == ["2ELb0", "2ELb1", "3ELb0", "3ELb1", "4ELb0", "4ELb1"]
