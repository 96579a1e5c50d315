"""(not gpu) Sweep 1's ring checks spill one chunk or none: the sweep kernels compiled by g++ (tests/cpp/hip_shim, as in
test_sweep_emulation.py) and run on the lines of tests/test_gpu_sweep_ring_checks.py -- the staircase that spills at every
check, the staircase interrupted, salt -- with 32-bit and 64-bit entries.  The kernel asserts the bound at every check
(tests/cpp/sweep_ring_checks.cc refuses to build without assertions), the driver counts the spills the lines must cause and
compares the results with a brute-force line transform.  In every ring / chunk size of test_sweep_emulation.py."""
import os
import subprocess

import pytest

from conftest import ROOT
from test_sweep_emulation import CONFIGS

CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.mark.parametrize("name,flags", CONFIGS)
def test_one_spill_per_check(name, flags):
    out = "sweep_ring_checks_" + name
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "sweep_ring_checks.mk", "RING_OUT=" + out, "SWEEP_FLAGS=" + flags])
    run = subprocess.run([os.path.join(CPP, out)], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-2000:]
    assert "\n0 failures" in run.stdout
    # the staircase of 1024 rows spills at (nearly) every check: the assertion stood on the path it guards
    assert "1024x1x65 scene 0" in run.stdout
