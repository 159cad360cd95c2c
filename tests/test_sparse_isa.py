"""Sparse renders and the upscaler's phase added kernels and changed none: the gfx950 assembly of every kernel the library had
before them — the trace kernels, the adaptive-pass kernels they are reached through, resolve_kernel, upscale_direct_kernel and all
the others — is what it was, instruction for instruction.

tests/golden/kernels_before_sparse.json holds, for each kernel of the build before this feature, the SHA-256 of its body as
`normalised` leaves it (comments and the function's number in its local labels dropped), recorded from that build with the
compiler the file names.  Another compiler lays the same source out differently: under one the comparison says nothing, and the
test says so instead of failing.  (upscale_direct_kernel's two entries were recorded again when §4.20's stage rule became
W >= 2^-40, a change of that kernel made on purpose.)"""
import hashlib
import json
import os
import re
import shutil
import subprocess

import pytest

import isa_asm

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernels_before_sparse.json")
NEW = ("sparse_check_kernel", "sparse_resolve_kernel", "upscale_phase_kernel")


def normalised(lines):
    out = []
    for l in lines:
        l = l.split(";")[0]  # (trailing comments name basic blocks by the function's number in the file)
        l = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", l)  # .. and so do its local labels
        l = " ".join(l.split())
        if l:
            out.append(l)
    return out


def digest(lines):
    return hashlib.sha256("\n".join(normalised(lines)).encode()).hexdigest()


def compiler():
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    text = subprocess.run([hipcc, "--version"], check=True, capture_output=True, text=True, timeout=60).stdout
    return " | ".join(l.strip() for l in text.split("\n") if re.match(r"^(HIP version|AMD clang version)", l.strip()))


@pytest.fixture(scope="module")
def kernels():
    golden = json.load(open(GOLDEN))
    if golden["compiler"] != compiler():
        pytest.skip(f"the recorded assembly is {golden['compiler']}'s; this is {compiler()}")
    return golden["kernels"], isa_asm.bodies(isa_asm.device_asm(), "")


def test_every_kernel_from_before_is_unchanged(kernels):
    before, now = kernels
    assert len(before) == 91
    for stem in ("trace_kernel", "flat_xy_kernel", "flat_one_radius_kernel", "primary_xz_kernel", "trace_kernel_bvh", "adaptive_pass_kernel",
                 "adaptive_pass_kernel_bvh", "resolve_kernel", "accumulate_kernel", "upscale_direct_kernel", "upscale_pack_var_kernel"):
        assert any(stem in k for k in before), stem
    missing = sorted(set(before) - set(now))
    assert not missing, missing
    changed = sorted(k for k in before if digest(now[k]) != before[k]["sha256"])
    assert not changed, changed
    assert all(len(normalised(now[k])) == before[k]["lines"] for k in before)


def test_the_new_kernels_are_the_only_new_ones(kernels):
    before, now = kernels
    added = sorted(set(now) - set(before))
    assert added and all(any(stem in k for stem in NEW) for k in added), added
    # one check kernel; the resolve per precision with and without the variance; the phase kernel with and without it
    assert [sum(stem in k for k in added) for stem in NEW] == [1, 4, 2]
    meta = isa_asm.metadata(isa_asm.device_asm())
    for k in added:
        print(k, "vgpr", meta[k]["vgpr_count"], "sgpr", meta[k]["sgpr_count"], "spills", meta[k]["vgpr_spill_count"], meta[k]["sgpr_spill_count"])
        assert int(meta[k]["vgpr_spill_count"]) == 0 and int(meta[k]["sgpr_spill_count"]) == 0 and int(meta[k]["private_segment_fixed_size"]) == 0
