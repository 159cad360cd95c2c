"""The device headers under rayz_device.hpp include what they use: each one parses as the first and only include of an empty HIP
source, with the library's flags, device side only, and without a warning: a template that names a function no included header
declares is accepted under -std=c++17 as a C++20 extension and only warned about, so that warning is an error here and no other is let through.  The list is
read from the umbrella's own #include lines, so a header added there later is covered, and the feature headers that stand on
them are held to the same; the umbrella itself holds nothing but comment and includes."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rayz_amd", "csrc")


def _umbrella_lines():
    with open(os.path.join(CSRC, "rayz_device.hpp")) as f:
        return f.read().split("\n")


UMBRELLA = [m.group(1) for m in (re.match(r'#include "([^"]+)"', line) for line in _umbrella_lines()) if m]
HEADERS = UMBRELLA + ["chain_kernel.hpp", "noise.hpp", "sparse.hpp", "adaptive.hpp", "temporal_modes_kernel.hpp"]  # device headers of features, outside the umbrella


def test_umbrella_holds_only_comment_and_includes():
    assert len(UMBRELLA) >= 11, UMBRELLA
    for line in _umbrella_lines():
        assert line == "" or line.startswith("//") or line == "#pragma once" or re.match(r'#include "[^"]+"\s*(//.*)?$', line), line


@pytest.mark.parametrize("header", HEADERS)
def test_header_parses_alone(header, tmp_path):
    from rayz_amd import _build

    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    assert os.path.exists(os.path.join(CSRC, header)), header
    src = tmp_path / "only.hip"
    src.write_text('#include "%s"\n' % header)
    run = subprocess.run([hipcc, *_build.HIPFLAGS, "-Werror=c++20-extensions", "-I", CSRC, "--cuda-device-only", "-fsyntax-only", str(src)], capture_output=True,
                         text=True, timeout=600)
    # (a warning at a source position; the driver's own note on an unused link flag has none)
    assert run.returncode == 0 and not re.search(r":\d+:\d+: warning:", run.stderr), run.stderr[-4000:]
