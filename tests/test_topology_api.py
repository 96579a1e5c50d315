"""(not gpu) The component-topology entry points of the C ABI exist, are bound, and reject bad arguments before any HIP
call, leaving their outputs untouched."""
import ctypes
import os

import numpy as np
import pytest

from voxelized_geometry_tools_amd import capi

NEW = ["vgt_hip_component_topology", "vgt_hip_component_topology_dev", "vgt_hip_cells_component_topology"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load()


def test_entry_points_are_bound_and_exported(lib):
    raw = ctypes.CDLL(capi.LIB_PATH)
    for name in NEW:
        assert name in capi.SIGNATURES and hasattr(raw, name), name
    assert lib.vgt_hip_abi_version() == 2
    assert capi.COMPONENT_TOPOLOGY.itemsize == 32
    assert capi.COMPONENT_TOPOLOGY.names == ("present", "num_holes", "num_voids", "num_surfaces", "m3", "m5", "m6",
                                             "num_surface_vertices")
    for method in (capi.Context.component_topology, capi.Context.component_topology_dev, capi.Cells.component_topology):
        assert callable(method)


def test_argument_errors_without_device(lib):
    """No context exists here (no device needed): every call must fail with code 1 and a message, touching nothing."""
    occ = np.zeros(8, np.float32)
    labels = np.zeros(8, np.uint32)
    table = np.zeros(9, capi.COMPONENT_TOPOLOGY)
    count = ctypes.c_uint32(12345)
    o, l, t = (capi._ptr(a) for a in (occ, labels, table))
    c = ctypes.byref(count)

    def dev(shape, types=7, ctx=None, components=1):
        return lib.vgt_hip_component_topology_dev(ctx, o, l, *shape, types, components, t)

    def host(shape, types=7, ctx=None):
        return lib.vgt_hip_component_topology(ctx, o, *shape, types, l, c, t, 9)

    for fn in (dev, host):
        assert fn((2, 2, 2)) == 1 and b"null" in lib.vgt_hip_last_error()
        for shape in ((0, 2, 2), (2, -1, 2), (2, 2, 0)):
            assert fn(shape) == 1 and b"positive" in lib.vgt_hip_last_error()
        for shape in ((2048, 1024, 1024), (1 << 40, 1 << 40, 1 << 40), (1, 1, 1 << 31)):
            assert fn(shape) == 1 and b"2^31" in lib.vgt_hip_last_error()
        # below 2^31 cells, but the vertex lattice is not
        for shape in ((1, 1, (1 << 31) - 2), (1290, 1290, 1290), (1, (1 << 30) - 1, 1)):
            assert shape[0] * shape[1] * shape[2] < (1 << 31) - 1
            assert fn(shape) == 1 and b"lattice" in lib.vgt_hip_last_error() and b"2^31" in lib.vgt_hip_last_error()
        for types in (0, 8, -1):
            assert fn((2, 2, 2), types) == 1 and b"component types" in lib.vgt_hip_last_error()
    assert dev((2, 2, 2), components=9) == 1 and b"more components than cells" in lib.vgt_hip_last_error()
    for types in (0, 8, -1):
        assert lib.vgt_hip_cells_component_topology(None, None, 0, types, l, c, t, 9) == 1
        assert b"component types" in lib.vgt_hip_last_error()
    assert lib.vgt_hip_cells_component_topology(None, None, 0, 7, l, c, t, 9) == 1 and b"null" in lib.vgt_hip_last_error()
    assert not labels.any() and count.value == 12345 and not any(table[f].any() for f in table.dtype.names)
