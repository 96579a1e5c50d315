"""(not gpu) The coarse-hull form of the plain X pass on the CPU: the sweep kernels compiled by g++ (tests/cpp/hip_shim, as
in test_sweep_emulation.py) run the X sweep with the coarse form on and off against a brute-force line transform on lines of
65, 96, 97, 128, 130, 512 and 1024 rows -- distance-like fields, salt, lines without any site or with one at row 0 or at the
last row, a subsample whose every row is "no site", inputs at the 22-bit limit, a one-class plane between planes that have
sites -- and tests/cpp/sweep_coarse_hull.cc asserts that every row the chord test drops is absent from the stack of the
unfiltered algorithm when its line ends.  In the ring and band sizes of test_sweep_emulation.py that keep chunks of eight
32-bit entries (the coarse area is laid out in such chunks)."""
import os
import subprocess

import pytest

from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")

CONFIGS = [
    ("default", ""),
    ("b8_r32_c8", "-DVGT_SWEEP_BAND=8 -DVGT_SWEEP_RING=32 -DVGT_SWEEP_CHUNK=8"),
    ("b32_r64_c8", "-DVGT_SWEEP_BAND=32 -DVGT_SWEEP_RING=64 -DVGT_SWEEP_CHUNK=8"),
]


@pytest.mark.parametrize("name,flags", CONFIGS)
def test_coarse_hull_on_cpu(name, flags):
    out = "sweep_coarse_hull_" + name
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "sweep_coarse_hull.mk", "COARSE_OUT=" + out, "SWEEP_FLAGS=" + flags])
    run = subprocess.run([os.path.join(CPP, out)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-2000:]
    assert "7 lengths" in run.stdout and " 0 failures" in run.stdout
    # (the filter was at work: rows were dropped and checked)
    assert int(run.stdout.split(" lengths, ")[1].split()[0]) > 1000
