"""The feed of the flat list's scan loops.  Each loop walks its stream with one running 64-bit pointer and loads
at constant offsets from it; every scalar load is issued right after a wait, into the SGPR set that is free, so that a whole
group's packed FMAs lie between a load and the wait that covers it; the reject branch is a scalar branch on a ballot.  ISA
checks of the two compiled f32 flat kernels (trace_kernel, adaptive_pass_kernel), found as tests/test_plane_runs.py finds the
loops, in each of the five packed loops (static plane, static loose, mov-Y plane, mov-Y loose, bucket):
  * at most 6 scalar ALU instructions per iteration (every s_* that is no load, wait or branch; s_nop counts);
  * no s_waitcnt with an lgkmcnt field within the 10 v_pk_fma_f32 that follow an s_load (around the back edge too);
  * no s_and_saveexec.
And one host check: how far a scan reads (rayz_amd/csrc/plane_runs.hpp: scan_reach, compiled into tests/scan_reach_mirror.cpp)
is what the loop's order of loads gives, restated here, and stays inside the two spare groups of every section the layout
mirrors (tests/plane_filter_mirror.cpp, tests/bucket_mirror.cpp) lay out for config 3 and for pools of short runs."""
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from rayz_amd import tracer
from test_plane_runs import G, ROOT, _groups, _run, _spheres, _write, mirror  # noqa: F401  (mirror: a fixture)
from test_speed_buckets import bmirror, pool, same, spread  # noqa: F401  (bmirror: a fixture)

HERE = os.path.dirname(os.path.abspath(__file__))
KERNELS = ["_ZN8rayz_dev12trace_kernelIfLi1EEEvNS_9TraceArgsIT_EE", "_ZN8rayz_dev20adaptive_pass_kernelIfLi1EEEvNS_9TraceArgsIT_EE"]
PACKED = [2 * 6 * G // 2, 2 * 7 * G // 2, 2 * 7 * G // 2, 2 * 8 * G // 2, 2 * 6 * G // 2]  # packed FMAs per iteration, slot order


@pytest.fixture(scope="module")
def device_asm(tmp_path_factory):
    from rayz_amd import _build

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    asm = tmp_path_factory.mktemp("scan_feed") / "dev.s"
    flags = [f for f in _build.HIPFLAGS if f not in ("-fPIC", "-Wall", "-Wextra")]
    subprocess.run([hipcc, *flags, "--cuda-device-only", "-S", "-o", str(asm), os.path.join(ROOT, "rayz_amd", "csrc", "rayz_hip.hip")],
                   check=True, capture_output=True, timeout=600)
    return asm.read_text()


def scan_loops(text, name):
    """The kernel's scan loops as lists of instructions (labels dropped): the innermost backward branches whose body holds
    packed FMAs, as tests/test_plane_runs.py finds them."""
    body = text[text.index(name + ":"):]
    body = [l for l in body[:body.index(".Lfunc_end")].split("\n") if l.strip() and not l.strip().startswith(";")]
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\w+):", l)] if m}
    loops = []
    for i, l in enumerate(body):
        m = re.search(r"s_cbranch_\w+ (\.LBB\w+)", l)
        if m and labels.get(m.group(1), i) < i and i - labels[m.group(1)] < 100:
            loop = [x.strip() for x in body[labels[m.group(1)]:i + 1] if not re.match(r"^\.LBB\w+:", x)]
            if any(x.startswith("v_pk_fma_f32") for x in loop):
                loops.append(loop)
    return loops


@pytest.mark.parametrize("kernel", KERNELS)
def test_packed_loops_feed_from_a_running_pointer_behind_covered_loads(device_asm, kernel):
    loops = scan_loops(device_asm, kernel)
    assert [sum(x.startswith("v_pk_fma_f32") for x in lp) for lp in loops[:5]] == PACKED, [len(lp) for lp in loops]
    for lp, pk in zip(loops[:5], PACKED):
        op = [x.split()[0] for x in lp]
        salu = [x for x, o in zip(lp, op) if o.startswith("s_") and not re.match(r"s_(load|buffer_load|waitcnt|cbranch|branch)", o)]
        print(kernel[13:35], pk, "packed FMAs:", len(lp), "instructions,", len(salu), "scalar ALU,",
              sum(o.startswith("s_load") for o in op), "s_load,", sum(o == "s_waitcnt" for o in op), "s_waitcnt")
        assert len(salu) <= 6, (pk, salu)
        assert not any(o.startswith("s_and_saveexec") for o in op), (pk, "a divergent reject branch")
        assert any(o.startswith("s_load") for o in op) and any(o == "s_waitcnt" and "lgkmcnt" in x for x, o in zip(lp, op))
        n = len(lp)
        for i, o in enumerate(op):
            if not o.startswith("s_load"):
                continue
            fmas, j = 0, i + 1
            while fmas < 10:  # the loop is a cycle: what follows its last instruction is its first
                x = lp[j % n]
                assert not (x.startswith("s_waitcnt") and "lgkmcnt" in x), (pk, f"`{lp[i]}` is waited for after {fmas} packed FMAs")
                fmas += x.startswith("v_pk_fma_f32")
                j += 1
                assert j - i <= 2 * n


def loaded_groups(first, end, group):
    """The groups (by first slot) the scan of slots [first, end) loads, in the loop's order (flat_scan.hpp: scan_blocks): the
    first group before the loop; per iteration, the pair's second group, then the first of the next pair."""
    at, out = first, [first]
    while at < end:
        out += [at + group, at + 2 * group]
        at += 2 * group
    return out


def test_no_scan_reads_past_its_sections_spare_groups(mirror, bmirror, tmp_path):
    gxx = shutil.which("g++")
    exe = str(tmp_path / "scan_reach_mirror")
    subprocess.run([gxx, "-std=c++17", "-O2", "-o", exe, os.path.join(HERE, "scan_reach_mirror.cpp")], check=True, capture_output=True, timeout=300)

    def reach(group, scans):
        r = subprocess.run([exe, str(group), *[str(v) for s in scans for v in s]], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stderr
        out = json.loads(r.stdout)
        assert out["spare_groups"] == 2
        return out["reach"]

    # the library's scan_reach is what the loop's loads give, at every length around whole group pairs (mov-G: groups of 2)
    for group in (G, 2):
        scans = [(f, f + n) for f in (0, 2 * group, 10 * group) for n in range(0, 5 * group + 1)]
        assert reach(group, scans) == [max(loaded_groups(f, e, group)) + group for f, e in scans]
    rng = np.random.default_rng(3)
    pools = [_spheres(tracer.randomBouncing(64, -50, 50, seed=42)), _spheres(tracer.randomBouncing(64, -5, 5, seed=42)),
             _groups([(0, 0.5, 64), (0, 1.5, 65), (0, 2.5, 72), (1, 0.5, 64), (1, 1.5, 71)], rng),
             pool([(0.5, 64, same(0.3)), (1.5, 73, same(-0.2)), (2.5, 200, spread(0.30, 0.32, rng))], rng)]
    checked = 0
    for sph in pools:
        sp = _write(tmp_path, "s.bin", sph)
        lay = _run(mirror, tmp_path, "layout", sp)["classes"]
        runs1 = _run(bmirror, tmp_path, "layout", sp)["runs"]
        for c in (0, 1):
            plane_section = lay[c]["plane_slots"] + 2 * G  # slots of the plane section, its two spare groups included
            scans = [(r["first"], r["end"]) for r in lay[c]["runs"]]
            if c == 1:  # a y-moving run's own loop starts behind its buckets' slots
                scans = [(r["first"] + r["bucketed"], r["end"]) for r in runs1 if r["first"] + r["bucketed"] < r["end"]]
            assert all(x <= plane_section for x in reach(G, scans)), (c, scans)
            n_loose = -(-len(lay[c]["loose"]) // (2 * G)) * 2 * G
            assert reach(G, [(0, n_loose)]) == [n_loose + G] and n_loose + G <= n_loose + 2 * G
            checked += len(scans) + 1
        # the bucket section: the buckets' blocks back to back in table order, then two spare groups
        sizes = [b["end"] - b["first"] for r in runs1 for b in r["buckets"]]
        at = np.concatenate([[0], np.cumsum(sizes)]).astype(int).tolist()
        assert all(x <= at[-1] + 2 * G for x in reach(G, list(zip(at[:-1], at[1:])))), sizes
        checked += len(sizes)
    n_movg = -(-6 // 4) * 4  # six spheres of general velocity: groups of 2, whole pairs, two spare groups
    assert reach(2, [(0, n_movg)])[0] <= n_movg + 2 * 2
    assert checked > 20
