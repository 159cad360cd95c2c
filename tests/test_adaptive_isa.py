"""The kernels of an adaptive pass (adaptive_pass_kernel, adaptive_pass_kernel_bvh: the text of trace_kernel / trace_kernel_bvh
compiled a second time over the active list) carry the same hazards as the product trace kernels and are held to
the same two properties of their gfx950 code as tests/test_isa_invariants.py holds those to: nothing touches the registers of a BVH
node load still in flight between the box step's two waits, and the kernels stay off the codegen cliffs (no vector spills in f32,
global and not flat loads in the BVH shading pass, the flat-list kernel's scalar spills inside the guarded limit).  Their names keep
them out of that file's `trace_kernel` patterns, which count exactly the six product kernels; hence this file."""
import re

import pytest

import isa_asm
from isa_asm import bodies


@pytest.fixture(scope="module")
def device_asm():
    return isa_asm.device_asm()


def test_no_instruction_touches_the_node_fetch_registers_in_flight(device_asm):
    kernels = bodies(device_asm, "adaptive_pass_kernel_bvh")
    assert len(kernels) == 4, sorted(kernels)  # f32 / f64 x two record formats
    blocks = 0
    for name, L in kernels.items():
        for i, line in enumerate(L):
            m = re.search(r"s_waitcnt vmcnt\((\d)\) lgkmcnt\((\d)\)", line)
            if not m or m.group(1) != m.group(2) or m.group(1) not in "12":
                continue
            n = int(m.group(1))  # loads still in flight after this wait: the last n of the fetch (global and LDS turn alike)
            dests, j = [], i - 1
            while j > 0 and i - j < 40:
                mm = re.search(r"(?:global_load_dwordx4|ds_read_b128) v\[(\d+):(\d+)\]", L[j])
                if mm:
                    dests.append((int(mm.group(1)), int(mm.group(2))))
                j -= 1
            assert len(dests) == 4 * n, (name, i, dests)  # both turns issue 2n loads each
            regs = set()
            for a, b in dests[:n] + dests[2 * n:3 * n]:  # the last n of either turn
                regs |= set(range(a, b + 1))
            k = i + 1
            while "s_waitcnt vmcnt(0) lgkmcnt(0)" not in L[k]:
                for a, b, c in re.findall(r"v\[(\d+):(\d+)\]|\bv(\d+)\b", L[k]):
                    used = {int(c)} if c else set(range(int(a), int(b) + 1))
                    assert not (used & regs), f"{name}: `{L[k].strip()}` touches a register of a node load still in flight"
                k += 1
                assert k - i < 80, (name, "no second wait after the split one")
            blocks += 1
    assert blocks >= 2 * 4  # two steps per wave-level decision in each kernel


def test_adaptive_pass_kernels_stay_off_their_codegen_cliffs(device_asm):
    meta = isa_asm.metadata(device_asm)
    passes = {k: v for k, v in meta.items() if "adaptive_pass_kernel" in k}
    assert len(passes) == 6, sorted(passes)  # flat f32 / f64, BVH f32 / f64 x two node-record formats
    for name, f in passes.items():
        f64 = "IdL" in name  # (TraceArgs<double>)
        assert int(f["vgpr_count"]) <= 128, (name, f["vgpr_count"])
        assert int(f["vgpr_spill_count"]) <= (1 if f64 else 0), (name, f["vgpr_spill_count"])
        if "bvh" not in name and not f64:
            assert int(f["sgpr_spill_count"]) <= 80, (name, f["sgpr_spill_count"])  # the product kernel's limit
    for name, L in bodies(device_asm, "adaptive_pass_kernel_bvh").items():
        assert not any(re.match(r"\s*flat_load", l) for l in L), f"{name}: a flat_load in the BVH kernel of an adaptive pass"
        assert not any(re.match(r"\s*scratch_(load|store)", l) for l in L) or "IdL" in name, f"{name}: scratch traffic in an f32 BVH kernel"
