"""The denoiser's kernels of both modes as compiled for gfx950 (cross-compiled, as tests/test_isa_invariants.py does): no vector
register spilled, no scratch, static LDS within 64 KiB, the records fetched with 16-byte loads — and names that stay out of the trace
kernels' count."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_denoise_kernels_codegen(tmp_path):
    from rayz_amd import _build

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    asm = tmp_path / "dev.s"
    flags = [f for f in _build.HIPFLAGS if f not in ("-fPIC", "-Wall", "-Wextra")]
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-o", str(asm), os.path.join(ROOT, "rayz_amd", "csrc", "rayz_hip.hip")],
                   check=True, capture_output=True, timeout=600)
    text = asm.read_text()
    meta = {}
    kernels = text[text.index("amdhsa.kernels:"):]
    for entry in re.split(r"\n  - (?=\.\w+:)", kernels)[1:]:  # one YAML list item per kernel; .args holds nested items, scalars are unique
        fields = dict(re.findall(r"^    \.(\w+):\s+(\S+)$", entry, flags=re.M))
        fields.update(re.findall(r"^\.(\w+):\s+(\S+)$", entry.split("\n")[0]))
        if "name" in fields:
            meta[fields["name"]] = fields
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
    name, body, bodies = None, [], {}
    for line in text.split("\n"):
        m = re.match(r"^(_ZN8rayz_dev\w*denoise_\w+):", line)
        if m:
            name, body = m.group(1), []
        elif name is not None:
            if line.startswith(".Lfunc_end"):
                bodies[name], name = body, None
            elif not line.lstrip().startswith(";"):
                body.append(line)
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
