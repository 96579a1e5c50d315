"""The mesh rasterizer of the C++ host layer (include/vgt_hip/mesh_rasterizer.hpp, csrc/host/hip_mesh_rasterizer.cc)
through tests/cpp/test_mesh_host.cc: the reference's two gtest cases and its two exceptions."""
import os
import subprocess

import pytest

from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
PKG = os.path.join(ROOT, "voxelized_geometry_tools_amd")
BINARY = os.path.join(CPP, "test_mesh_host")


def _build():
    if not os.path.exists(os.path.join(PKG, "libvgt_hip.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(PKG, "csrc")])
    subprocess.check_call(["make", "-s", "-C", CPP, os.path.join("..", "..", "voxelized_geometry_tools_amd",
                                                                 "libvgt_hip_host.so")])
    subprocess.check_call(["make", "-s", "-C", os.path.join(PKG, "csrc", "host")])
    source = os.path.join(CPP, "test_mesh_host.cc")
    newest = max(os.path.getmtime(p) for p in (source, os.path.join(PKG, "libvgt_hip_mesh_host.so")))
    if os.path.exists(BINARY) and os.path.getmtime(BINARY) >= newest:
        return
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           "-o", BINARY, source, "-L" + PKG, "-lvgt_hip_mesh_host", "-lvgt_hip_host", "-lvgt_hip",
                           "-Wl,-rpath,$ORIGIN/../../voxelized_geometry_tools_amd"])


def test_errors_without_device():
    _build()
    out = subprocess.run([BINARY, "--no-device"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASSED" in out.stdout


@pytest.mark.gpu
def test_reference_cases_through_cpp_layer():
    _build()
    out = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout
