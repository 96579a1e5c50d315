"""SurfaceIndices, the display exports and ExtractComponentSurfaces of the C++ host layer (include/vgt_hip/) through
tests/cpp/test_display_host.cc, built by the rule tests/cpp/Makefile has for its test binaries."""
import os
import subprocess

import pytest

from conftest import ROOT

CPP = os.path.join(ROOT, "tests", "cpp")
BINARY = os.path.join(CPP, "test_display_host")


def _build():
    pkg = os.path.join(ROOT, "voxelized_geometry_tools_amd")
    if not os.path.exists(os.path.join(pkg, "libvgt_hip.so")):
        subprocess.check_call(["make", "-s", "-j4", "-C", os.path.join(pkg, "csrc")])
    subprocess.check_call(["make", "-s", "-C", CPP, "BINARIES=test_display_host", "test_display_host"])


def test_argument_errors_without_device():
    _build()
    out = subprocess.run([BINARY, "--no-device"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASSED" in out.stdout


def test_the_sanitizer_build_of_the_host_layer_takes_the_new_source():
    """tests/cpp/Makefile compiles every csrc/host/hip_*.cc into test_hip_host_asan (host code only, never device code)."""
    listing = subprocess.check_output(["make", "-n", "-B", "-C", CPP, "test_hip_host_asan"], text=True)
    assert "hip_display.cc" in listing and "-fsanitize=address" in listing


def test_the_host_library_exports_the_display_layer():
    _build()
    lib = os.path.join(ROOT, "voxelized_geometry_tools_amd", "libvgt_hip_host.so")
    symbols = subprocess.check_output(["nm", "-DC", "--defined-only", lib], text=True)
    for name in ("SurfaceIndices", "ExportForDisplay", "ExportForSeparateDisplay", "ExportSurfacesForDisplay"):
        for cell in ("DenseGrid", "CellGrid<vgt_hip::OccupancyComponentCell>", "CellGrid<vgt_hip::TaggedObjectOccupancyCell>",
                     "CellGrid<vgt_hip::TaggedObjectOccupancyComponentCell>"):
            assert any(("vgt_hip::%s(vgt_hip::%s const&" % (name, cell)) in line for line in symbols.splitlines()), \
                (name, cell)
    for name in ("ExportConnectedComponentsForDisplay", "ExportSDFForDisplay", "ExportSDFForDisplayCollisionOnly",
                 "ExtractComponentSurfaces"):
        assert "vgt_hip::%s(" % name in symbols, name


@pytest.mark.gpu
def test_display_through_cpp_layer(sdf_kats):
    _build()
    case = next(c for c in sdf_kats["extrema_cases"] if c["name"] == "CenterObstacle")
    assert case["shape"] == [4, 8, 12]
    args = [str(v) for v in case["shape"]] + [repr(case["resolution"])] + [str(v) for v in case["filled_box"]]
    out = subprocess.run([BINARY] + args, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout
