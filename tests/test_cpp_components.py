"""The component entry points of the C++ host layer (UpdateConnectedComponents, UpdateSpatialSegments,
ExtractComponentSurfaces; include/vgt_hip/hip_pointcloud_voxelizer.hpp) through tests/cpp/test_components_host.cc
(built by tests/cpp/Makefile)."""
import os
import subprocess

import pytest

from conftest import ROOT
from cpp_build import build

BINARY = os.path.join(ROOT, "tests", "cpp", "test_components_host")


def _build():
    build("test_components_host")


def test_argument_errors_without_device():
    _build()
    out = subprocess.run([BINARY, "--no-device"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASSED" in out.stdout


@pytest.mark.gpu
def test_components_through_cpp_layer():
    _build()
    out = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout
