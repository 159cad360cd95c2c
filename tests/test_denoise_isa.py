"""The denoiser's kernels of both modes as compiled for gfx950 (cross-compiled, as tests/test_isa_invariants.py does): no vector
register spilled, no scratch, static LDS within 64 KiB, the records fetched with 16-byte loads — and names that stay out of the trace
kernels' count."""
import re

import isa_asm


def test_denoise_kernels_codegen():
    text = isa_asm.device_asm()
    meta = isa_asm.metadata(text)
    dn = {k: v for k, v in meta.items() if "denoise_" in k}
    # {plain, guided} x (pack + direct x {level, last} + LDS x {stride 1, 2, 4} x {level, last})
    assert len(dn) == 2 * (1 + 2 + 6), sorted(dn)
    assert sum("_pack_" in k for k in dn) == 2 and sum("_direct_" in k for k in dn) == 4 and sum("_lds_" in k for k in dn) == 12, sorted(dn)
    lds_sizes = set()
    for name, f in dn.items():
        assert "trace_kernel" not in name
        assert int(f["vgpr_spill_count"]) == 0 and int(f["sgpr_spill_count"]) == 0, (name, f)
        assert int(f["private_segment_fixed_size"]) == 0, (name, f["private_segment_fixed_size"])  # no scratch
        assert int(f["group_segment_fixed_size"]) <= 64 * 1024, (name, f["group_segment_fixed_size"])
        assert int(f["vgpr_count"]) <= 128, (name, f["vgpr_count"])  # 4 waves per SIMD or better
        if "_lds_" in name:
            lds_sizes.add(int(f["group_segment_fixed_size"]))
        else:
            assert int(f["group_segment_fixed_size"]) == 0, name
    # (32 + 4S) x (8 + 4S) records of 48 bytes for S = 1, 2, 4
    assert lds_sizes == {36 * 12 * 48, 40 * 16 * 48, 48 * 24 * 48}, lds_sizes
    # the bodies: records move 16 bytes at a time, nothing goes through flat or scratch instructions
    bodies = isa_asm.bodies(text, "denoise_")
    assert set(bodies) == set(dn)
    for name, L in bodies.items():
        ops = [l.split()[0] for l in L if l.strip() and not l.strip().endswith(":")]
        assert not any(o.startswith(("scratch_", "flat_")) for o in ops), name
        if "level" in name:
            assert ops.count("global_load_dwordx4") >= 3, name
            assert not any(o in ("global_load_dword", "global_load_dwordx2", "global_load_dwordx3") for o in ops), name
        if "_lds_" in name:
            assert ops.count("ds_read_b128") >= 3 and "ds_write_b128" in ops, name
            assert not any(o.startswith("ds_read_b32") or o.startswith("ds_read2") for o in ops), name
