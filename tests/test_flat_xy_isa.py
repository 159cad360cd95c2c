"""The compiled f32 flat_xy_kernel (trace_kernels_flat.hpp: trace_kernel_flat.hpp once more, with the reject test's xy basis, DESIGN.md
§4.3, §6): what its five packed scan loops must look like on gfx950, found as tests/test_scan_feed.py finds trace_kernel's.
  * packed FMAs per iteration (two groups of G spheres, two spheres per v_pk_fma_f32): 5 per sphere pair in the static plane loop
    and the bucket loop, 7 in the mov-Y plane remainder, 7 on loose static spheres, 9 on loose y-moving ones;
  * no loop reads a spilled register (v_readlane, scratch_) or takes a divergent reject branch (s_and_saveexec);
  * at most 6 scalar ALU instructions per iteration;
  * a whole group's packed FMAs lie between each s_load and the lgkmcnt wait that covers it: half the loop's packed FMAs, i.e.
    10 in the 5-FMA loops, 14 in the 7-FMA loops, 18 in the 9-FMA loop;
  * the kernel: at most 128 VGPRs, no VGPR spill, at most 80 SGPR spills (trace_kernel's own limits)."""
import re

import isa_asm

G = 4  # device_types.hpp: group_size<float>()
F32 = "_ZN8rayz_dev14flat_xy_kernelIfLi1EEEvNS_9TraceArgsIT_EE"
F64 = "_ZN8rayz_dev14flat_xy_kernelIdLi1EEEvNS_9TraceArgsIT_EE"
PER_PAIR = [5, 7, 7, 9, 5]  # static plane, static loose, mov-Y plane, mov-Y loose, bucket: the scan's order
PACKED = [2 * n * G // 2 for n in PER_PAIR]


def scan_loops(text, name):
    """The kernel's scan loops as lists of instructions: the innermost backward branches whose body holds packed FMAs."""
    body = isa_asm.bodies(text, "flat_xy_kernel")[name]
    body = [l for l in body if l.strip()]
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\w+):", l)] if m}
    loops = []
    for i, l in enumerate(body):
        m = re.search(r"s_cbranch_\w+ (\.LBB\w+)", l)
        if m and labels.get(m.group(1), i) < i and i - labels[m.group(1)] < 100:
            loop = [x.strip() for x in body[labels[m.group(1)]:i + 1] if not re.match(r"^\.LBB\w+:", x)]
            # a packed block loop: at least two packed FMAs per sphere pair of its 2·G spheres (the general-velocity loop tests
            # its spheres with scalar FMAs, of which the compiler may pair a few)
            if sum(x.startswith("v_pk_fma_f32") for x in loop) >= 2 * G:
                loops.append(loop)
    return loops


def test_the_kernel_exists_once_per_precision_under_a_name_of_its_own():
    meta = isa_asm.metadata(isa_asm.device_asm())
    mine = sorted(k for k in meta if "flat_xy_kernel" in k)
    assert mine == sorted([F32, F64]), mine
    assert not any("trace_kernel" in k or "adaptive_pass_kernel" in k for k in mine)


def test_kernel_registers_and_spills():
    f = isa_asm.metadata(isa_asm.device_asm())[F32]
    print("flat_xy_kernel<float>: vgpr", f["vgpr_count"], "vgpr spills", f["vgpr_spill_count"], "sgpr spills", f["sgpr_spill_count"])
    assert int(f["vgpr_count"]) <= 128
    assert int(f["vgpr_spill_count"]) == 0
    assert int(f["sgpr_spill_count"]) <= 80


def test_packed_loops_five_seven_seven_nine_five():
    loops = scan_loops(isa_asm.device_asm(), F32)
    assert [sum(x.startswith("v_pk_fma_f32") for x in lp) for lp in loops[:5]] == PACKED, [len(lp) for lp in loops]
    for lp, pk in zip(loops[:5], PACKED):
        op = [x.split()[0] for x in lp]
        salu = [x for x, o in zip(lp, op) if o.startswith("s_") and not re.match(r"s_(load|buffer_load|waitcnt|cbranch|branch)", o)]
        print(pk, "packed FMAs:", len(lp), "instructions,", sum(o.startswith("v_") for o in op), "VALU,", len(salu), "scalar ALU,",
              sum(o.startswith("s_load") for o in op), "s_load,", sum(o == "s_waitcnt" for o in op), "s_waitcnt")
        assert not any("v_readlane" in x or "scratch_" in x for x in lp), (pk, "a spilled register is read in a scan loop")
        assert not any(o.startswith("s_and_saveexec") for o in op), (pk, "a divergent reject branch")
        assert len(salu) <= 6, (pk, salu)
        assert any(o.startswith("s_load") for o in op) and any(o == "s_waitcnt" and "lgkmcnt" in x for x, o in zip(lp, op))
        n, group = len(lp), pk // 2  # a whole group's packed FMAs behind every load, before the wait that covers it
        for i, o in enumerate(op):
            if not o.startswith("s_load"):
                continue
            fmas, j = 0, i + 1
            while fmas < group:  # the loop is a cycle: what follows its last instruction is its first
                x = lp[j % n]
                assert not (x.startswith("s_waitcnt") and "lgkmcnt" in x), (pk, f"`{lp[i]}` is waited for after {fmas} packed FMAs")
                fmas += x.startswith("v_pk_fma_f32")
                j += 1
                assert j - i <= 2 * n
