"""The cells kernels (trace_kernels_flat.hpp: trace_kernel_flat.hpp with RAYZ_TRACE_KERNEL_CELLS, the three scan forms with every listable
segment resolved from the slab's cells) added kernels and changed none.

  * tests/golden/kernels_before_cells.json holds, for each kernel of the build before them, the SHA-256 of its body as
    test_sparse_isa.normalised leaves it, recorded from that build with the compiler the file names: every one is what it was,
    instruction for instruction and label for label.  (Another compiler lays the same source out differently: under one the
    comparison says nothing, and the test says so instead of failing.)  The four upscale_direct_kernel / upscale_phase_kernel
    entries were recorded again when §4.20's stage rule became W >= 2^-40, a change of those kernels made on purpose.
  * The six new kernels — one per scan form and precision — are the only new ones, under names no other ISA test counts and in
    a namespace of their own, rayz_dev_cells (tests/test_sparse_isa.py takes every kernel of rayz_dev that its record lacks for a
    sparse-render kernel).
  * The f32 ones keep within 128 VGPRs.  Their list phase does cost spills outside the scan loops, which trace_kernel has none of:
    at most 26 VGPR spills (2 / 10 / 26 for XZ / XY / ONE_RADIUS) and 44 bytes of scratch a lane.
  * Their scan loops carry the packed-FMA counts of the kernels they were made from, loop by loop, in f32 and f64, and none reads
    a spilled register (v_readlane, scratch_): the query's f64 temporaries are dead before the scan starts."""
import json
import os
import re

import pytest

import isa_asm
from test_primary_lists_isa import G, kernel, scan_loops
from test_sparse_isa import compiler, digest, normalised

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernels_before_cells.json")
MADE_FROM = {"cells_xz_kernel": "trace_kernel", "cells_xy_kernel": "flat_xy_kernel", "cells_one_radius_kernel": "flat_one_radius_kernel"}


def cells_kernel(stem, r):
    """The mangled name of rayz_dev_cells::stem<R, 1> (R: "f" or "d")."""
    names = [k for k in isa_asm.metadata(isa_asm.device_asm()) if re.match(rf"_ZN14rayz_dev_cells\d+{stem}I{r}Li1EEEvN8rayz_dev14CellsTraceArgsIT_EE$", k)]
    assert len(names) == 1, (stem, r, names)
    return names[0]


def cells_scan_loops(text, name):
    """test_primary_lists_isa.scan_loops for a kernel outside rayz_dev: the straight-line stretches that hold a whole iteration's packed
    FMAs and end in the reject branch."""
    lines = text[text.index("\n" + name + ":"):]
    lines = lines[:lines.index(".Lfunc_end")].split("\n")[2:]
    loops, run = [], []
    for l in lines:
        x = l.strip()
        if not x or x.startswith(";"):
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


@pytest.fixture(scope="module")
def kernels():
    golden = json.load(open(GOLDEN))
    if golden["compiler"] != compiler():
        pytest.skip(f"the recorded assembly is {golden['compiler']}'s; this is {compiler()}")
    return golden["kernels"], isa_asm.bodies(isa_asm.device_asm(), "")


def test_every_kernel_from_before_is_unchanged(kernels):
    before, now = kernels
    assert len(before) == 98
    for stem in ("trace_kernel", "flat_xy_kernel", "flat_one_radius_kernel", "primary_xz_kernel", "primary_one_radius_kernel", "primary_lists_kernel",
                 "adaptive_pass_kernel", "sparse_resolve_kernel", "trace_kernel_bvh", "resolve_kernel"):
        assert any(stem in k for k in before), stem
    missing = sorted(set(before) - set(now))
    assert not missing, missing
    changed = sorted(k for k in before if digest(now[k]) != before[k]["sha256"])
    assert not changed, changed
    assert all(len(normalised(now[k])) == before[k]["lines"] for k in before)


def test_the_cells_kernels_are_the_only_new_ones(kernels):
    before, now = kernels
    assert sorted(now) == sorted(before)  # rayz_dev holds what it held ..
    meta = isa_asm.metadata(isa_asm.device_asm())
    added = sorted(k for k in meta if "rayz_dev_cells" in k or "cells_" in k)  # .. and the new namespace the six
    assert added == sorted(cells_kernel(stem, r) for stem in MADE_FROM for r in "fd"), added
    for k in added:
        assert not any(s in k for s in ("trace_kernel", "flat_xy_kernel", "flat_one_radius_kernel", "adaptive_pass_kernel", "primary_")), k


@pytest.mark.parametrize("stem", sorted(MADE_FROM))
def test_f32_registers_and_spills(stem):
    f = isa_asm.metadata(isa_asm.device_asm())[cells_kernel(stem, "f")]
    print(f"{stem}<float>: vgpr", f["vgpr_count"], "vgpr spills", f["vgpr_spill_count"], "sgpr spills", f["sgpr_spill_count"], "scratch",
          f["private_segment_fixed_size"])
    assert int(f["vgpr_count"]) <= 128
    assert int(f["vgpr_spill_count"]) <= 26 and int(f["private_segment_fixed_size"]) <= 44  # outside the scan loops (below)
    assert int(f["sgpr_spill_count"]) <= 96


@pytest.mark.parametrize("r", ["f", "d"])
@pytest.mark.parametrize("stem", sorted(MADE_FROM))
def test_the_scan_loops_are_those_of_the_kernel_it_was_made_from(stem, r):
    text = isa_asm.device_asm()
    mine = cells_scan_loops(text, cells_kernel(stem, r))
    parent = scan_loops(text, MADE_FROM[stem], kernel(MADE_FROM[stem], r))
    count = lambda loops: [sum(x.startswith("v_pk_fma_f32") for x in lp) for lp in loops]  # noqa: E731
    print(stem, r, count(mine))
    assert len(parent) >= 5 and count(mine) == count(parent), (count(mine), count(parent))
    for lp in mine:
        assert not any("v_readlane" in x or "scratch_" in x for x in lp), (stem, r, "a spilled register is read in a scan loop")
