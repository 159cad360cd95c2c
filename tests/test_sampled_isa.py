"""The sampled G-buffer kernels (sampled_kernel.hpp) as compiled for gfx950: six kernels — the flat-list one for
f32 and f64, the BVH one for f32 and f64 over either node format — all in rayz_dev_sampled, none under rayz_dev's prefix (whose
kernel set test_sparse_isa.py and test_slab_cells_isa.py hold to their records); no vector register spilled and no scratch frame;
registers and scalar spills at most what DESIGN.md §6 records.  The figures were read from the code object of the compiler named
below; another compiler allocates differently, and under one the bounds say nothing, so the test says so instead of failing."""
import os
import re
import shutil
import subprocess

import pytest

import isa_asm

COMPILER = ("HIP version: 7.2.26015-fc0010cf6a | AMD clang version 22.0.0git (https://github.com/RadeonOpenCompute/llvm-project roc-7.2.0 26014 "
            "7b800a19466229b8479a78de19143dc33c3ab9b5)")
PREFIX = "_ZN16rayz_dev_sampled"
# kernel: (VGPRs, SGPR spills) as measured; VGPR spills and scratch bytes are 0 for all six
MEASURED = {
    "14sampled_kernelIfEE": (97, 32),
    "14sampled_kernelIdEE": (93, 179),
    "18sampled_kernel_bvhIfLb0EEE": (107, 2),
    "18sampled_kernel_bvhIfLb1EEE": (107, 8),
    "18sampled_kernel_bvhIdLb0EEE": (111, 25),
    "18sampled_kernel_bvhIdLb1EEE": (111, 27),
}


def compiler():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    text = subprocess.run([hipcc, "--version"], check=True, capture_output=True, text=True, timeout=60).stdout
    return " | ".join(l.strip() for l in text.split("\n") if re.match(r"^(HIP version|AMD clang version)", l.strip()))


@pytest.fixture(scope="module")
def meta():
    if compiler() != COMPILER:
        pytest.skip(f"the recorded figures are {COMPILER}'s; this is {compiler()}")
    return isa_asm.metadata(isa_asm.device_asm())


def test_the_six_kernels_live_in_their_own_namespace(meta):
    mine = sorted(k for k in meta if "sampled" in k)
    assert len(mine) == 6 and all(k.startswith(PREFIX) for k in mine), mine
    assert not [k for k in mine if k.startswith("_ZN8rayz_dev")]
    for stem in MEASURED:
        assert sum(k.startswith(PREFIX + stem) for k in mine) == 1, (stem, mine)
    # .. and rayz_dev gained no function of theirs that stopped being inlined
    assert not [k for k in isa_asm.bodies(isa_asm.device_asm(), "") if "ampled" in k]


def test_registers_spills_and_scratch(meta):
    for stem, (vgprs, sgpr_spills) in MEASURED.items():
        k = next(k for k in meta if k.startswith(PREFIX + stem))
        m = meta[k]
        print(k, "vgpr", m["vgpr_count"], "sgpr", m["sgpr_count"], "spills", m["vgpr_spill_count"], m["sgpr_spill_count"], "scratch",
              m["private_segment_fixed_size"], "lds", m["group_segment_fixed_size"])
        assert int(m["vgpr_spill_count"]) == 0 and int(m["private_segment_fixed_size"]) == 0, k
        assert int(m["vgpr_count"]) <= vgprs and int(m["sgpr_spill_count"]) <= sgpr_spills, k
        assert int(m["vgpr_count"]) <= 128 and int(m.get("agpr_count", 0)) == 0, k  # (four waves per SIMD, as the chain kernels)
        assert int(m["group_segment_fixed_size"]) == 0, k  # (the BVH kernels' LDS is dynamic: the render's layout)


def test_the_header_parses_alone(tmp_path):
    """As tests/test_device_headers_cpu.py holds the headers of its list."""
    from rayz_amd import _build

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(isa_asm.ROOT, "rayz_amd", "csrc")
    src = tmp_path / "only.hip"
    src.write_text('#include "sampled_kernel.hpp"\n')
    run = subprocess.run([hipcc, *_build.HIPFLAGS, "-Werror=c++20-extensions", "-I", csrc, "--cuda-device-only", "-fsyntax-only", str(src)],
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0 and not re.search(r":\d+:\d+: warning:", run.stderr), run.stderr[-4000:]
