"""(not gpu) Sweep 2's per-band choice between its two copies of the band code (csrc/edt_sweep_kernels.hip): the kernel
source compiled by g++ against the host stand-in for the HIP runtime, as tests/test_sweep_emulation.py does, and run by
tests/cpp/sweep_class_bands.cc on lines built so that bands that may drop the class-change candidates and bands that
must keep them lie next to each other -- both passes, 32-bit and 64-bit entries, bands of 8 and of 16 rows, against the
brute-force line contract.  The kernel tallies the bands by the copy they ran; both outcomes must be frequent."""
import os
import re
import subprocess

import pytest

from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
# (the compile line of tests/cpp/Makefile's sweep emulation)
COMPILE = ["g++", "-O2", "-std=c++17", "-x", "c++", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unused-function",
           "-Wno-unknown-pragmas", "-Ihip_shim", "-I" + os.path.join(ROOT, "include")]


@pytest.mark.parametrize("band", [8, 16])
def test_class_band_choice_on_cpu(band):
    out = "sweep_emulation_class_bands_b%d" % band
    subprocess.check_call(COMPILE + ["-DVGT_SWEEP_BAND=%d" % band, "-o", out, "sweep_class_bands.cc"], cwd=CPP)
    run = subprocess.run([os.path.join(CPP, out)], capture_output=True, text=True, timeout=600)
    print(run.stdout)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-2000:]
    assert " 0 mismatches" in run.stdout
    assert "(band %d)" % band in run.stdout
    for name in ("Y", "X"):
        m = re.search(r"%s pass: (\d+) bands with candidates after the second vote, (\d+) without candidates, "
                      r"(\d+) with candidates after the first vote" % name, run.stdout)
        assert m, run.stdout
        second, skipped, first = (int(v) for v in m.groups())
        # a condition on the test's own lines, not a measurement: both outcomes occur, often, in each pass
        assert skipped >= 1000, (name, skipped)
        assert second + first >= 1000, (name, second, first)
        assert second >= 100, (name, second)
