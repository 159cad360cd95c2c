#!/usr/bin/env python3
"""Which gfx950 kernels does a change touch?  Compiles rayz_hip.hip device-only to assembly in two trees and compares per symbol.

  python tools/isa_diff.py OLD NEW [--allow REGEX ...]     OLD, NEW: a source tree, or a git revision of this repository
  python tools/isa_diff.py HEAD .  --allow '^void rayz_dev::kat_kernel<'

Comments and the per-compilation __hip_cuid symbol are dropped, labels lose their function's number (and a long branch's
.Lpost_getpc label its number in the file, which every kernel added in front of it shifts); the text is split at each function's .type line (what
precedes the first is "(preamble)", the code objects' notes are "(metadata)").  Prints every symbol that differs with the number
of changed lines, and exits 1 if one of them matches no --allow pattern (patterns are searched in the demangled name).
"""
import argparse, difflib, os, re, shutil, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rayz_amd._build import HIPFLAGS, _hipcc  # noqa: E402


def assembly(tree: str, tmp: str, tag: str) -> dict[str, list[str]]:
    if not os.path.isdir(tree):  # a git revision: its files, unpacked
        rev, tree = tree, os.path.join(tmp, tag)
        os.makedirs(tree)
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "rayz_amd", "include"], check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tree], input=tar, check=True)
    out = os.path.join(tmp, tag + ".s")
    subprocess.run([_hipcc(), *HIPFLAGS, "--cuda-device-only", "-S", "-o", out, os.path.join(tree, "rayz_amd", "csrc", "rayz_hip.hip")], check=True)
    # (labels carry the function's number in the file, and so do the comments behind a label: both go)
    lines = [re.sub(r"\.(LBB|Lfunc_begin|Lfunc_end|Lpost_getpc)\d+", r".\1", l if '"' in l else re.sub(r"\s*;.*", "", l))
             for l in open(out) if l.strip() and not l.lstrip().startswith(";") and "__hip_cuid" not in l]
    notes = next((i for i, l in enumerate(lines) if l.lstrip().startswith(".amdgpu_metadata")), len(lines))
    parts: dict[str, list[str]] = {}
    name = "(preamble)"
    for line in lines[:notes]:
        m = re.match(r"\s*\.type\s+([^,\s]+),@function", line)
        if m:  # the directives that open this function's section stand in front of its .type line: they go with it
            prev, name, head = parts.get(name, []), m.group(1), []
            while prev and re.match(r"\s*\.(section|text|protected|globl|weak|hidden|p2align)\b", prev[-1]):
                head.insert(0, prev.pop())
            parts.setdefault(name, []).extend(head)
        parts.setdefault(name, []).append(line)
    # the code object's notes: one list entry ("  - ") per kernel, which goes with that kernel's code; the rest is "(metadata)"
    for entry in re.split(r"(?m)^(?=  - )", "".join(lines[notes:])):
        m = re.search(r"(?m)^    \.symbol:\s+(\S+)\.kd$", entry)
        parts.setdefault(m.group(1) if m else "(metadata)", []).extend(entry.splitlines(True))
    return parts


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--allow", action="append", default=[], metavar="REGEX", help="a symbol that may differ (demangled name)")
    ap.add_argument("--keep", metavar="DIR", help="leave old.s and new.s (and an unpacked revision) in DIR, which must be empty")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(2) as pool:
        tmp = args.keep or tmp
        a, b = pool.map(assembly, (args.old, args.new), (tmp, tmp), ("old", "new"))
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    syms = sorted(a.keys() | b.keys())
    pretty = subprocess.run([filt], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n") if filt else syms
    bad = same = 0
    for sym, nice in zip(syms, pretty):
        if a.get(sym) == b.get(sym):
            same += 1
            continue
        how = "only in OLD" if sym not in b else "only in NEW" if sym not in a else "%d lines differ" % sum(
            l[0] in "+-" and l[:3] not in ("+++", "---") for l in difflib.unified_diff(a[sym], b[sym], n=0))
        allowed = any(re.search(p, nice) for p in args.allow)
        bad += not allowed
        print("%s  %s: %s" % ("allowed " if allowed else "DIFFERS ", nice, how))
    print("%d symbols identical, %d differ, %d of them not allowed" % (same, len(syms) - same, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
