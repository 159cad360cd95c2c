"""The compiled f32 flat_one_radius_kernel (trace_kernels_flat.hpp: trace_kernel_flat.hpp once more, the xy basis with the one-radius
sets in scan_sets' loop): what its scan loops must look like on gfx950, found as tests/test_flat_xy_isa.py finds
flat_xy_kernel's.
  * the five loops flat_xy_kernel has, with its packed-FMA counts (5, 7, 7, 9, 5 per sphere pair over two groups of 4), and the set
    loop once per class, behind the static loose loop and behind the bucket loop: 5 per sphere pair over two groups of 8, so 40;
  * the set loop: one s_load_dwordx16 per group of 8 and nothing else loaded (no r² field), one lgkmcnt wait per group, a whole
    group's 20 packed FMAs between each load and the wait that covers it, 8 of its packed FMAs with R2 as their scalar operand,
    one reject branch per 16 tests, at most 6 scalar ALU instructions;
  * no loop reads a spilled register (v_readlane, scratch_), waits on s_nop or takes a divergent reject branch (s_and_saveexec);
  * the kernel: at most 128 VGPRs, no VGPR spill, at most 80 SGPR spills (trace_kernel's own limits)."""
import re

import isa_asm

G, GS = 4, 8  # device_types.hpp: group_size<float>(); plane_runs.hpp: kSetGroup
F32 = "_ZN8rayz_dev22flat_one_radius_kernelIfLi1EEEvNS_9TraceArgsIT_EE"
F64 = "_ZN8rayz_dev22flat_one_radius_kernelIdLi1EEEvNS_9TraceArgsIT_EE"
# static plane, static loose, static sets, mov-Y plane, mov-Y loose, bucket, mov-Y sets: the scan's order
PACKED = [5 * G, 7 * G, 5 * GS, 7 * G, 9 * G, 5 * G, 5 * GS]


def scan_loops(text, name):
    """The kernel's scan loops as lists of instructions: the innermost backward branches whose body holds packed FMAs."""
    body = [l for l in isa_asm.bodies(text, "flat_one_radius_kernel")[name] if l.strip()]
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\w+):", l)] if m}
    loops = []
    for i, l in enumerate(body):
        m = re.search(r"s_cbranch_\w+ (\.LBB\w+)", l)
        if m and labels.get(m.group(1), i) < i and i - labels[m.group(1)] < 120:
            loop = [x.strip() for x in body[labels[m.group(1)]:i + 1] if not re.match(r"^\.LBB\w+:", x)]
            if sum(x.startswith("v_pk_fma_f32") for x in loop) >= 2 * G:
                loops.append(loop)
    return loops


def test_the_kernel_exists_once_per_precision_under_a_name_of_its_own():
    meta = isa_asm.metadata(isa_asm.device_asm())
    mine = sorted(k for k in meta if "flat_one_radius_kernel" in k)
    assert mine == sorted([F32, F64]), mine
    assert not any("trace_kernel" in k or "flat_xy_kernel" in k or "adaptive_pass_kernel" in k for k in mine)


def test_kernel_registers_and_spills():
    f = isa_asm.metadata(isa_asm.device_asm())[F32]
    print("flat_one_radius_kernel<float>: vgpr", f["vgpr_count"], "vgpr spills", f["vgpr_spill_count"], "sgpr spills", f["sgpr_spill_count"])
    assert int(f["vgpr_count"]) <= 128
    assert int(f["vgpr_spill_count"]) == 0
    assert int(f["sgpr_spill_count"]) <= 80


def test_the_loops_and_the_set_loop_among_them():
    loops = scan_loops(isa_asm.device_asm(), F32)
    assert [sum(x.startswith("v_pk_fma_f32") for x in lp) for lp in loops[:7]] == PACKED, [len(lp) for lp in loops]
    for lp, pk in zip(loops[:7], PACKED):
        op = [x.split()[0] for x in lp]
        salu = [x for x, o in zip(lp, op) if o.startswith("s_") and not re.match(r"s_(load|buffer_load|waitcnt|cbranch|branch|nop)", o)]
        print(pk, "packed FMAs:", len(lp), "instructions,", sum(o.startswith("v_") for o in op), "VALU,", len(salu), "scalar ALU,",
              sum(o.startswith("s_load") for o in op), "s_load,", sum(o == "s_waitcnt" for o in op), "s_waitcnt")
        assert not any("v_readlane" in x or "scratch_" in x for x in lp), (pk, "a spilled register is read in a scan loop")
        assert not any(o.startswith("s_and_saveexec") for o in op), (pk, "a divergent reject branch")
        assert len(salu) <= 6, (pk, salu)
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
    for lp in (loops[2], loops[6]):  # the set loop
        op = [x.split()[0] for x in lp]
        assert "s_nop" not in op, lp
        loads = [x for x in lp if x.startswith("s_load")]
        assert len(loads) == 2 and all(x.startswith("s_load_dwordx16") for x in loads), loads  # cx[8] cz[8] in one load: no r² field
        assert sum(o == "s_waitcnt" for o in op) == 2 and sum(o.startswith("s_cbranch") for o in op) == 2  # (the reject branch, the loop's)
        # R2: ONE scalar operand for the eight disc FMAs, the third source of fm(−p2, p2, R2)
        r2 = [re.search(r"(s\[\d+:\d+\]) neg_lo", x).group(1) for x in lp if x.startswith("v_pk_fma_f32") and re.search(r"s\[\d+:\d+\] neg_lo", x)]
        assert len(r2) == GS and len(set(r2)) == 1, r2
        held = int(re.match(r"s\[(\d+):", r2[0]).group(1))  # .. and loop-invariant: outside both sets the loads fill
        for x in loads:
            lo, hi = map(int, re.match(r"s_load_dwordx16 s\[(\d+):(\d+)\]", x).groups())
            assert not lo <= held <= hi, (r2[0], x)


def test_f64_kernel_keeps_its_scratch_out_of_the_scan_loops():
    """The f64 instantiation spills (128 VGPRs, a few bytes of scratch, SGPRs to lanes): none of it inside a scan loop, the set loop
    included, which has the f32 kernel's counts (the reject test is f32 for both precisions)."""
    text = isa_asm.device_asm()
    f = isa_asm.metadata(text)[F64]
    print("flat_one_radius_kernel<double>: vgpr", f["vgpr_count"], "scratch bytes", f["private_segment_fixed_size"], "sgpr spills", f["sgpr_spill_count"])
    assert int(f["vgpr_count"]) <= 128 and int(f["private_segment_fixed_size"]) <= 16
    loops = scan_loops(text, F64)
    assert [sum(x.startswith("v_pk_fma_f32") for x in lp) for lp in loops[:7]] == PACKED, [len(lp) for lp in loops]
    for lp in loops[:7]:
        assert not any("v_readlane" in x or "v_writelane" in x or "scratch_" in x or x.startswith("s_nop") for x in lp), lp
