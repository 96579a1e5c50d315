"""The C++ host layer (include/vgt_hip/, csrc/host/) -- the part a maintainer of the reference
would actually link -- exercised by tests/cpp/test_hip_host.cc, a restatement of the
reference's sdf_generation_test / pointcloud_voxelization_test against that layer."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT
from cpp_build import build

BINARY = os.path.join(ROOT, "tests", "cpp", "test_hip_host")


def _build():
    build("test_hip_host")


def test_backend_unavailable_behaviour():
    """(not gpu) helper constructs but reports unavailable for an impossible device; the
    voxelizer constructor throws runtime_error; option validation throws invalid_argument."""
    _build()
    out = subprocess.run([BINARY, "--no-device"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "PASSED" in out.stdout


GLUE_SRC = os.path.join(ROOT, "voxelized_geometry_tools_amd", "csrc", "host", "hip_voxelization_helpers.cc")
PLUGIN_SYMBOLS = os.path.join(ROOT, "tests", "golden", "plugin_boundary_symbols.json")


def plugin_boundary_symbols(include_dirs=()):
    """Mangled names of the plugin boundary in the glue's object file: the interface classes, their handles, vtables and
    type info, and every override of HipVoxelizationHelper (its signatures are spelled out in the names).  AvailableDevice's
    inline constructor is left out: the stand-alone declarations take its arguments by value, the reference's header by
    const reference (source-compatible, inline on both sides)."""
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        obj = os.path.join(tmp, "glue.o")
        subprocess.check_call(["g++", "-std=c++17", "-O0", "-fPIC", "-Wall", "-c", GLUE_SRC, "-o", obj] +
                              ["-I" + d for d in include_dirs])
        mangled = sorted({line.split()[-1] for line in
                          subprocess.run(["nm", obj], capture_output=True, text=True, check=True).stdout.splitlines()
                          if line.strip()})
    demangled = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True,
                               check=True).stdout.splitlines()
    keep = ("DeviceVoxelizationHelperInterface", "TrackingGridsHandle", "FilterGridHandle", "HipVoxelizationHelper")
    out = []
    for m, d in zip(mangled, demangled):
        owner = d.replace("(anonymous namespace)", "{anonymous}").split("(")[0]
        if not (d.startswith("voxelized_geometry_tools::") or d.startswith(("vtable for voxelized_geometry_tools::",
                                                                             "typeinfo for voxelized_geometry_tools::",
                                                                             "typeinfo name for voxelized_geometry_tools::"))):
            continue
        if any(k in owner for k in keep) and "AvailableDevice" not in owner and " std::" not in owner:
            out.append(m)
    return out


def test_glue_compiles_against_reference_header():
    """(not gpu) the glue is written against the reference's own device_voxelization_interface.hpp: compiled stand-alone
    (the declarations of include/vgt_hip/voxelization_plugin_api.hpp), its plugin-boundary symbols are exactly those it
    had when compiled with the reference's header on the include path (tests/golden/plugin_boundary_symbols.json, recorded
    by `python tests/test_cpp_host.py --record-plugin-symbols <reference>/include`)."""
    with open(PLUGIN_SYMBOLS) as fh:
        want = json.load(fh)["symbols"]
    got = plugin_boundary_symbols()
    assert len(want) > 40
    assert got == want, {"missing": sorted(set(want) - set(got)), "extra": sorted(set(got) - set(want))}


@pytest.mark.gpu
def test_reference_suites_through_cpp_layer():
    _build()
    out = subprocess.run([BINARY], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    assert "PASSED" in out.stdout


if __name__ == "__main__":
    # python tests/test_cpp_host.py --record-plugin-symbols <reference checkout>/include
    if len(sys.argv) != 3 or sys.argv[1] != "--record-plugin-symbols":
        raise SystemExit("usage: python tests/test_cpp_host.py --record-plugin-symbols <reference include dir>")
    ref_include = sys.argv[2]
    if not os.path.isfile(os.path.join(ref_include, "voxelized_geometry_tools", "device_voxelization_interface.hpp")):
        raise SystemExit("%s holds no voxelized_geometry_tools/device_voxelization_interface.hpp" % ref_include)
    doc = {"note": "plugin-boundary symbols of csrc/host/hip_voxelization_helpers.cc compiled with the reference's "
                   "include/ on the include path (g++ -std=c++17 -O0; tests/test_cpp_host.py)",
           "symbols": plugin_boundary_symbols([ref_include])}
    with open(PLUGIN_SYMBOLS, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print("%d symbols -> %s" % (len(doc["symbols"]), PLUGIN_SYMBOLS))
