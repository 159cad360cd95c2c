"""The compiled primary_xz_kernel, primary_xy_kernel and primary_one_radius_kernel (trace_kernels_flat.hpp: trace_kernel_flat.hpp with
RAYZ_TRACE_KERNEL_PRIMARY, the three scan forms with the camera segments from the pixels' primary lists) on gfx950:
  * each exists once per precision under a name of its own, none of which the ISA tests of the other trace kernels count, and
    primary_lists_kernel exists once;
  * the f32 ones: at most 128 VGPRs, no VGPR spill, at most 80 SGPR spills (trace_kernel's own limits);
  * their scan loops carry the packed-FMA counts of the kernels they were made from (trace_kernel, flat_xy_kernel,
    flat_one_radius_kernel), loop by loop, in f32 and f64;
  * no scan loop reads a spilled register (v_readlane, scratch_)."""
import re

import pytest

import isa_asm

G = 4  # device_types.hpp: group_size<float>()
MADE_FROM = {"primary_xz_kernel": "trace_kernel", "primary_xy_kernel": "flat_xy_kernel", "primary_one_radius_kernel": "flat_one_radius_kernel"}


def kernel(stem, r):
    """The mangled name of stem<R, 1> (R: "f" or "d"), found among the kernels whose name holds the stem."""
    names = [k for k in isa_asm.metadata(isa_asm.device_asm()) if re.match(rf"_ZN8rayz_dev\d+{stem}I{r}Li1EEEvNS_\d+\w*TraceArgsIT_EE$", k)]
    assert len(names) == 1, (stem, r, names)
    return names[0]


def scan_loops(text, stem, name):
    """The bodies of the kernel's scan loops, each from its header to its reject branch: the straight-line stretches that hold a
    whole iteration's packed FMAs (at least 5 per sphere pair of two groups) and end in a wave-uniform branch.  Found by stretch
    and not by backward branch: where the compiler lays a loop's counter block in front of its header the loop is the same."""
    loops, run = [], []
    for l in isa_asm.bodies(text, stem)[name]:
        x = l.strip()
        if not x:
            continue
        if re.match(r"^\.LBB\w+:", x):
            run = []
            continue
        run.append(x)
        if re.match(r"s_(cbranch|branch)", x):
            if x.startswith("s_cbranch_vcc") and sum(y.startswith("v_pk_fma_f32") for y in run) >= 5 * G:
                loops.append(run)
            run = []
    return loops


def test_the_kernels_exist_once_per_precision_under_names_of_their_own():
    meta = isa_asm.metadata(isa_asm.device_asm())
    mine = sorted(k for k in meta if "primary_" in k and "TraceArgs" in k)
    assert mine == sorted(kernel(stem, r) for stem in MADE_FROM for r in "fd"), mine
    for k in mine:
        assert not any(s in k for s in ("trace_kernel", "flat_xy_kernel", "flat_one_radius_kernel", "adaptive_pass_kernel")), k
    assert sum("primary_lists_kernel" in k for k in meta) == 1


@pytest.mark.parametrize("stem", sorted(MADE_FROM))
def test_f32_registers_and_spills(stem):
    f = isa_asm.metadata(isa_asm.device_asm())[kernel(stem, "f")]
    print(f"{stem}<float>: vgpr", f["vgpr_count"], "vgpr spills", f["vgpr_spill_count"], "sgpr spills", f["sgpr_spill_count"])
    assert int(f["vgpr_count"]) <= 128
    assert int(f["vgpr_spill_count"]) == 0
    assert int(f["sgpr_spill_count"]) <= 80


@pytest.mark.parametrize("r", ["f", "d"])
@pytest.mark.parametrize("stem", sorted(MADE_FROM))
def test_the_scan_loops_are_those_of_the_kernel_it_was_made_from(stem, r):
    text = isa_asm.device_asm()
    mine = scan_loops(text, stem, kernel(stem, r))
    parent = scan_loops(text, MADE_FROM[stem], kernel(MADE_FROM[stem], r))
    count = lambda loops: [sum(x.startswith("v_pk_fma_f32") for x in lp) for lp in loops]  # noqa: E731
    print(stem, r, count(mine))
    assert len(parent) >= 5 and count(mine) == count(parent), (count(mine), count(parent))
    for lp in mine:
        assert not any("v_readlane" in x or "scratch_" in x for x in lp), (stem, r, "a spilled register is read in a scan loop")
