"""The mesh rasterizer of the C++ host layer (include/vgt_hip/mesh_rasterizer.hpp, csrc/host/hip_mesh_rasterizer.cc)
through tests/cpp/test_mesh_host.cc: the reference's two gtest cases and its two exceptions."""
import os
import subprocess

import pytest

from conftest import ROOT
from cpp_build import build

BINARY = os.path.join(ROOT, "tests", "cpp", "test_mesh_host")


def _build():
    build("test_mesh_host")


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
