"""The device code of rayz_hip.hip as gfx950 assembly, for the tests that read it (test_isa_invariants.py, test_adaptive_isa.py,
test_denoise_isa.py, test_temporal_moments_isa.py, test_temporal_feedback_isa.py): one cross-compile per set of defines and pytest
process, the kernels' metadata and their bodies."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def device_asm(*defines: str) -> str:
    """The assembly text of the product's device code, built with the library's flags and `defines` ("-DNAME", ..)."""
    from rayz_amd import _build

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    flags = [f for f in _build.HIPFLAGS if f not in ("-fPIC", "-Wall", "-Wextra")]
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "dev.s")
        subprocess.run([hipcc, *flags, *defines, "--cuda-device-only", "-S", "-o", asm, os.path.join(ROOT, "rayz_amd", "csrc", "rayz_hip.hip")],
                       check=True, capture_output=True, timeout=600)
        with open(asm) as f:
            return f.read()


def metadata(asm: str):
    """amdhsa.kernels as {kernel name: {field: value}} of its scalar fields (vgpr_count, group_segment_fixed_size, ..)."""
    meta = {}
    kernels = asm[asm.index("amdhsa.kernels:"):]
    for entry in re.split(r"\n  - (?=\.\w+:)", kernels)[1:]:  # one YAML list item per kernel; .args holds nested items, scalars are unique
        fields = dict(re.findall(r"^    \.(\w+):\s+(\S+)$", entry, flags=re.M))
        fields.update(re.findall(r"^\.(\w+):\s+(\S+)$", entry.split("\n")[0]))
        if "name" in fields:
            meta[fields["name"]] = fields
    return meta


def bodies(asm: str, stem: str):
    """{kernel name: its lines without comment lines} of the rayz_dev kernels whose name contains `stem`."""
    out, name, body = {}, None, []
    for line in asm.split("\n"):
        m = re.match(r"^(_ZN8rayz_dev\w*" + stem + r"\w*):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
            elif not line.lstrip().startswith(";"):
                body.append(line)
    return out
