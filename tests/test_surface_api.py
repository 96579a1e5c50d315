"""(not gpu) The surface extraction entry points of the C ABI exist, are bound, and reject bad arguments before any HIP
call, through the product library."""
import ctypes
import os

import numpy as np
import pytest

from voxelized_geometry_tools_amd import capi

NEW = ["vgt_hip_extract_surface", "vgt_hip_extract_surface_dev", "vgt_hip_cells_extract_surface"]


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
    assert lib.vgt_hip_abi_version() == 2                                  # purely additive
    for name in ("extract_surface", "extract_surface_dev"):
        assert callable(getattr(capi.Context, name))
    assert callable(capi.Cells.extract_surface)
    header = open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "vgt_hip.h")).read()
    for name in NEW:
        assert header.count(name + "(") == 1


def test_argument_errors_without_device(lib):
    """No context exists here (no device needed): every call must fail with code 1 and a message, touching nothing."""
    values = np.full((4, 4, 4), 0.25, np.float32)
    vertices = np.full((8, 3), 7.0, np.float64)
    cells = np.full(8, 7, np.int32)
    triangles = np.full((8, 3), 7, np.int32)
    nv, nt = ctypes.c_int64(-7), ctypes.c_int64(-7)
    v = capi._ptr(values)
    for fn in (lib.vgt_hip_extract_surface, lib.vgt_hip_extract_surface_dev):
        def call(ctx=v, field=v, shape=(4, 4, 4), iso=0.0, resolution=0.5, vertices=vertices, cells=cells, vcap=8,
                 triangles=triangles, tcap=8, counts=(ctypes.byref(nv), ctypes.byref(nt))):
            # (a non-null context pointer is never dereferenced before the other checks: the field's address stands in)
            return fn(ctx, field, *shape, iso, 0, resolution, None, capi._ptr(vertices), capi._ptr(cells), vcap,
                      capi._ptr(triangles), tcap, *counts)

        def message():
            return lib.vgt_hip_last_error()

        assert call(ctx=None) == 1 and b"null" in message()
        assert call(field=None) == 1 and b"null" in message()
        assert call(counts=(None, ctypes.byref(nt))) == 1 and b"null" in message()
        assert call(counts=(ctypes.byref(nv), None)) == 1 and b"null" in message()
        for shape in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
            assert call(shape=shape) == 1 and b"positive" in message()
        for shape in ((1 << 11, 1 << 10, 1 << 10), (1 << 31, 1, 1), (1, 1 << 40, 1), (1 << 30, 1 << 30, 1 << 30)):
            assert call(shape=shape) == 1 and b"2^31" in message()
        for resolution in (0.0, -0.5, float("inf"), float("nan")):
            assert call(resolution=resolution) == 1 and b"resolution" in message()
        for iso in (float("nan"), float("inf"), float("-inf")):
            assert call(iso=iso) == 1 and b"iso" in message()
        assert call(vertices=None, cells=None, vcap=0) == 1 and b"triangle buffer needs a vertex buffer" in message()
        assert call(vertices=None, vcap=0, triangles=None, tcap=0) == 1 and b"cell buffer needs" in message()
        assert call(vertices=None, cells=None, triangles=None, tcap=0) == 1 and b"capacity" in message()
        assert call(triangles=None) == 1 and b"capacity" in message()
        assert call(vcap=-1) == 1 and call(tcap=-1) == 1
    assert lib.vgt_hip_cells_extract_surface(None, v, 0.5, None, None, None, 0, None, 0, ctypes.byref(nv),
                                             ctypes.byref(nt)) == 1 and b"null" in lib.vgt_hip_last_error()
    assert lib.vgt_hip_cells_extract_surface(v, None, 0.5, None, None, None, 0, None, 0, ctypes.byref(nv),
                                             ctypes.byref(nt)) == 1 and b"null" in lib.vgt_hip_last_error()
    assert (nv.value, nt.value) == (-7, -7)
    assert (vertices == 7.0).all() and (cells == 7).all() and (triangles == 7).all()


def test_a_grid_without_cubes_is_an_empty_mesh_and_launches_nothing(lib):
    """An extent of 1: success with 0 and 0 before the context is looked into (the pointer given here is no context)."""
    values = np.zeros((1, 5, 5), np.float32)
    v = capi._ptr(values)
    for fn in (lib.vgt_hip_extract_surface, lib.vgt_hip_extract_surface_dev):
        for shape in ((1, 5, 5), (5, 1, 5), (5, 5, 1)):
            nv, nt = ctypes.c_int64(-7), ctypes.c_int64(-7)
            assert fn(v, v, *shape, 0.0, 0, 0.5, None, None, None, 0, None, 0, ctypes.byref(nv), ctypes.byref(nt)) == 0
            assert (nv.value, nt.value) == (0, 0)
