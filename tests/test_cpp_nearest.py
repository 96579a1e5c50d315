"""ExtractNearestCells of the C++ host layer (include/vgt_hip/nearest_cells.hpp) through
tests/cpp/test_nearest_host.cc, built by the rule tests/cpp/Makefile has for its test binaries."""
import os
import subprocess

import pytest

from conftest import ROOT

BINARY = os.path.join(ROOT, "tests", "cpp", "test_nearest_host")


def _build():
    """tests/cpp/Makefile builds the binaries it lists in BINARIES by one pattern rule (which also brings the host layer's
    library up to date); this binary is not in that list, so the list is given on the command line."""
    pkg = os.path.join(ROOT, "voxelized_geometry_tools_amd")
    if not os.path.exists(os.path.join(pkg, "libvgt_hip.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(pkg, "csrc")])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "BINARIES=test_nearest_host",
                           "test_nearest_host"])


def test_argument_errors_without_device():
    _build()
    out = subprocess.run([BINARY, "--no-device"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASSED" in out.stdout


@pytest.mark.gpu
def test_nearest_through_cpp_layer():
    _build()
    out = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout
