"""KinematicChain and SolveInverseKinematics of the C++ host layer (include/vgt_hip/inverse_kinematics.hpp) through
tests/cpp/test_ik_host.cc, built by the rule tests/cpp/Makefile has for its test binaries.  Its --no-device mode (the chain
finder against hand-written chains, the argument errors) also runs once under AddressSanitizer +
UndefinedBehaviorSanitizer as a stand-alone CPU program: nothing loaded into python is sanitized."""
import glob
import os
import subprocess

import pytest

from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
PKG = os.path.join(ROOT, "voxelized_geometry_tools_amd")
BINARY = os.path.join(CPP, "test_ik_host")


def _build():
    """tests/cpp/Makefile builds the binaries it lists in BINARIES by one pattern rule (which also brings the host layer's
    library up to date); this binary is not in that list, so the list is given on the command line."""
    if not os.path.exists(os.path.join(PKG, "libvgt_hip.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(PKG, "csrc")])
    subprocess.check_call(["make", "-s", "-C", CPP, "BINARIES=test_ik_host", "test_ik_host"])


def test_chain_finder_and_argument_errors_without_device():
    _build()
    out = subprocess.run([BINARY, "--no-device"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASSED" in out.stdout


def test_chain_finder_and_argument_checks_under_sanitizers():
    """The host layer's sources are compiled into the program (as tests/cpp/Makefile does for test_hip_host_asan); the
    device library is linked as it is and no device is touched."""
    libasan = subprocess.run(["gcc", "-print-file-name=libasan.so"], capture_output=True, text=True).stdout.strip()
    if not os.path.isabs(libasan) or not os.path.exists(libasan):
        pytest.skip("libasan not available")
    if not os.path.exists(os.path.join(PKG, "libvgt_hip.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(PKG, "csrc")])
    binary = BINARY + "_asan"
    sources = sorted(glob.glob(os.path.join(PKG, "csrc", "host", "hip_*.cc")))
    assert os.path.join(PKG, "csrc", "host", "hip_inverse_kinematics.cc") in sources
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-O1", "-g",
                           "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), "-o", binary,
                           os.path.join(CPP, "test_ik_host.cc")] + sources +
                          ["-L" + PKG, "-lvgt_hip", "-Wl,-rpath," + PKG])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    out = subprocess.run([binary, "--no-device"], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    assert "PASSED" in out.stdout


@pytest.mark.gpu
def test_inverse_kinematics_through_cpp_layer():
    _build()
    out = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout
