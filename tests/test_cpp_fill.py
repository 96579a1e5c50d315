"""FillEnclosedSpace and the ...Solid... mesh functions of the C++ host layer (include/vgt_hip/) through
tests/cpp/test_fill_host.cc, built by the rule tests/cpp/Makefile has for its test binaries."""
import os
import subprocess

import pytest

from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
BINARY = os.path.join(CPP, "test_fill_host")


def _build():
    """tests/cpp/Makefile builds the binaries it lists in BINARIES by one pattern rule (which also brings the host layer's
    library up to date); this binary is not in that list, so the list is given on the command line."""
    pkg = os.path.join(ROOT, "voxelized_geometry_tools_amd")
    if not os.path.exists(os.path.join(pkg, "libvgt_hip.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(pkg, "csrc")])
    subprocess.check_call(["make", "-s", "-C", CPP, "BINARIES=test_fill_host", "test_fill_host"])


def test_argument_errors_without_device():
    _build()
    out = subprocess.run([BINARY, "--no-device"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASSED" in out.stdout


def test_the_sanitizer_build_of_the_host_layer_takes_the_new_source():
    """tests/cpp/Makefile compiles every csrc/host/hip_*.cc into test_hip_host_asan (host code only, never device code)."""
    listing = subprocess.check_output(["make", "-n", "-B", "-C", CPP, "test_hip_host_asan"], text=True)
    assert "hip_fill_enclosed.cc" in listing and "-fsanitize=address" in listing


@pytest.mark.gpu
def test_fill_through_cpp_layer():
    _build()
    out = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout
