"""(not gpu) The component entry points of the C ABI exist, are bound, and reject bad arguments before any HIP call."""
import ctypes
import math
import os

import numpy as np
import pytest

from voxelized_geometry_tools_amd import capi

NEW = ["vgt_hip_connected_components", "vgt_hip_connected_components_dev", "vgt_hip_cells_connected_components",
       "vgt_hip_cells_spatial_segments", "vgt_hip_cells_spatial_segments_dev", "vgt_hip_cells_update_spatial_segments",
       "vgt_hip_component_surface_mask", "vgt_hip_component_surface_mask_dev"]


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


def test_argument_errors_without_device(lib):
    """No context exists here (no device needed): every call must fail with code 1 and a message, touching nothing."""
    occ = np.zeros(8, np.float32)
    labels = np.zeros(8, np.uint32)
    mask = np.zeros(8, np.uint8)
    extrema = np.zeros(24, np.float64)
    count = ctypes.c_uint32(0)
    o, l, m, e = (capi._ptr(a) for a in (occ, labels, mask, extrema))
    c = ctypes.byref(count)
    for fn in (lib.vgt_hip_connected_components, lib.vgt_hip_connected_components_dev):
        assert fn(None, o, 2, 2, 2, l, c) == 1 and b"null" in lib.vgt_hip_last_error()
        for shape in ((0, 2, 2), (2, -1, 2), (2, 2, 0)):
            assert fn(None, o, *shape, l, c) == 1 and b"positive" in lib.vgt_hip_last_error()
        for shape in ((2048, 1024, 1024), (1 << 40, 1 << 40, 1 << 40), (1, 1, 1 << 31)):
            assert fn(None, o, *shape, l, c) == 1 and b"2^31" in lib.vgt_hip_last_error()
    assert lib.vgt_hip_cells_connected_components(None, None, 0, l, c) == 1 and b"null" in lib.vgt_hip_last_error()
    for bad in (math.nan, -1.0, -math.inf):
        assert lib.vgt_hip_cells_spatial_segments(None, None, e, bad, l, c) == 1
        assert b"threshold" in lib.vgt_hip_last_error()
        assert lib.vgt_hip_cells_spatial_segments_dev(None, None, e, bad, l, c) == 1
        assert b"threshold" in lib.vgt_hip_last_error()
        assert lib.vgt_hip_cells_update_spatial_segments(None, None, bad, 0.1, 1, 0, None, l, c) == 1
        assert b"threshold" in lib.vgt_hip_last_error()
    assert lib.vgt_hip_cells_spatial_segments(None, None, e, 1.0, l, c) == 1 and b"null" in lib.vgt_hip_last_error()
    assert lib.vgt_hip_cells_spatial_segments_dev(None, None, e, 1.0, l, c) == 1
    assert lib.vgt_hip_cells_update_spatial_segments(None, None, 1.0, 0.1, 1, 0, None, l, c) == 1
    for fn in (lib.vgt_hip_component_surface_mask, lib.vgt_hip_component_surface_mask_dev):
        for types in (0, 8, -1):
            assert fn(None, o, l, 2, 2, 2, types, m) == 1 and b"component types" in lib.vgt_hip_last_error()
        assert fn(None, o, l, 2, 0, 2, 7, m) == 1 and b"positive" in lib.vgt_hip_last_error()
        assert fn(None, o, l, 2, 2, 2, 7, m) == 1 and b"null" in lib.vgt_hip_last_error()
    assert not labels.any() and not mask.any() and count.value == 0
