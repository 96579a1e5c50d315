"""The one build recipe of the tests/test_cpp_*.py modules: a target of tests/cpp/Makefile (a test binary of the C++ host
layer; the Makefile brings the layer's library up to date first)."""
import os
import subprocess

from conftest import ROOT


def build(target):
    """Makes tests/cpp/<target>; builds libvgt_hip.so first when it is missing."""
    pkg = os.path.join(ROOT, "voxelized_geometry_tools_amd")
    if not os.path.exists(os.path.join(pkg, "libvgt_hip.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(pkg, "csrc")])
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), target])
