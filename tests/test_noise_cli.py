"""The `rayz` command line's optional `--until <rel_error>` (render until converged, rayz_hip_progressive_run_until): the argument
is checked before any device is touched, and without it the program prints what it always printed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "rayz_amd", "host", "rayz")
RATE = r"Finished render \(\d+\.\d\ds\): \d+\.\d\d rps and \d+\.\d\d us per ray\n"


def rayz(args, **env):
    return subprocess.run([EXE] + args, capture_output=True, env=dict(os.environ, RAYZ_SEED="7", RAYZ_BOUNCES="6", **env), timeout=600)


@pytest.mark.parametrize("args", [["96", "--until"], ["--until", "zero", "96"], ["96", "--until", "0"], ["96", "--until", "-0.1"],
                                  ["96", "--until", "nan"], ["96", "--until", "0.1x"]])
def test_a_bad_until_argument_is_refused_before_any_device(built, args):
    r = rayz(args)
    assert r.returncode == 2 and r.stderr == b"error: --until needs a positive relative error\n" and r.stdout == b""


def test_until_with_several_devices_is_refused(built):
    r = rayz(["96", "--until", "0.1"], RAYZ_DEVICES="0,1")
    assert r.returncode == 2 and b"--until renders on one device" in r.stderr and r.stdout == b""
    assert rayz(["--until", "0.1"]).returncode == 2  # the image width is still required


@pytest.mark.gpu
def test_until_stops_early_and_the_plain_output_is_unchanged(gpu, tmp_path):
    a, b, c = tmp_path / "a.ppm", tmp_path / "b.ppm", tmp_path / "c.ppm"
    plain = rayz(["96", str(a)], RAYZ_SPP="256")
    assert plain.returncode == 0 and re.fullmatch(RATE, plain.stderr.decode()), plain.stderr  # the rate line and nothing else
    # a threshold no pixel can meet: the schedule ends, the frame is the plain one, the line says so; the flag may stand anywhere
    full = rayz(["--until", "1e-9", "96", str(b)], RAYZ_SPP="256")
    assert full.returncode == 0, full.stderr
    assert re.fullmatch(RATE + r"Stopped at 256 of 256 samples per pixel: \d+\.\d\d% of the pixels above 1e-09 relative error\n",
                        full.stderr.decode()), full.stderr
    assert a.read_bytes() == b.read_bytes()
    early = rayz(["96", str(c), "--until", "0.5"], RAYZ_SPP="256")
    assert early.returncode == 0, early.stderr
    m = re.fullmatch(RATE + r"Stopped at (\d+) of 256 samples per pixel: (\d+\.\d\d)% of the pixels above 0.5 relative error\n", early.stderr.decode())
    assert m, early.stderr
    assert 16 < int(m.group(1)) < 256 and int(m.group(1)) % 16 == 0 and float(m.group(2)) <= 1.0  # passes of 16: at least two
    assert c.read_bytes().startswith(b"P3\n96 54\n")
