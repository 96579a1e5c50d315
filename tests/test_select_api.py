"""(not gpu) The cell-selection entry points of the C ABI exist, are bound, and reject bad arguments before any HIP
call."""
import ctypes
import os

import numpy as np
import pytest

from voxelized_geometry_tools_amd import capi

NEW = ["vgt_hip_select_cells", "vgt_hip_select_cells_dev", "vgt_hip_cells_select"]


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
    for name in ("select_cells", "select_cells_dev", "cells_select"):
        assert callable(getattr(capi.Context, name))
    assert callable(capi.Cells.select)
    assert (capi.SELECT_ALL, capi.SELECT_SURFACE_26, capi.SELECT_COMPONENT_SURFACE) == (0, 1, 2)
    assert (capi.CLASS_ABOVE, capi.CLASS_BELOW, capi.CLASS_EQUAL, capi.CLASS_UNORDERED) == (1, 2, 4, 8)
    header = open(os.path.join(os.path.dirname(capi._HERE), "include", "vgt_hip.h")).read()
    for name in ("SELECT_ALL", "SELECT_SURFACE_26", "SELECT_COMPONENT_SURFACE", "CLASS_ABOVE", "CLASS_BELOW",
                 "CLASS_EQUAL", "CLASS_UNORDERED", "CELL_MEMBER_NONE", "CELL_MEMBER_OBJECT_ID", "CELL_MEMBER_COMPONENT",
                 "CELL_MEMBER_SPATIAL_SEGMENT"):
        assert "#define VGT_HIP_%s 0x%02x\n" % (name, getattr(capi, name)) in header or \
            "#define VGT_HIP_%s %d\n" % (name, getattr(capi, name)) in header, name


def test_argument_errors_without_device(lib):
    """No context exists here (no device needed): every call must fail with code 1 and a message, touching nothing."""
    values = np.full((4, 4, 4), 0.25, np.float32)
    labels = np.ones((4, 4, 4), np.uint32)
    indices = np.full(64, -9, np.int32)
    out_values = np.full(64, -9.0, np.float32)
    out_labels = np.full(64, 9, np.uint32)
    count = ctypes.c_int64(-7)
    v, lab = capi._ptr(values), capi._ptr(labels)
    for fn in (lib.vgt_hip_select_cells, lib.vgt_hip_select_cells_dev):
        def call(ctx=v, values=v, labels=lab, shape=(4, 4, 4), rule=0, mask=15, t=0.5, indices=capi._ptr(indices),
                 ov=capi._ptr(out_values), ol=capi._ptr(out_labels), capacity=64, count=ctypes.byref(count)):
            # (a non-null context pointer is never dereferenced before the other checks: the values' address stands in)
            return fn(ctx, values, labels, *shape, rule, mask, t, indices, ov, ol, capacity, count)

        def message():
            return lib.vgt_hip_last_error()

        assert call(ctx=None) == 1 and b"null" in message()
        assert call(values=None) == 1 and b"null" in message()
        assert call(count=None) == 1 and b"null" in message()
        for rule in (-1, 3, 4, 0x10, 0x101):
            assert call(rule=rule) == 1 and b"rule" in message()
        for mask in (0, 16, -1, 0x1f):
            assert call(mask=mask) == 1 and b"class mask" in message()
        assert call(rule=2, labels=None, ol=None) == 1 and b"needs labels" in message()
        assert call(rule=0, labels=None) == 1 and b"needs labels" in message()          # a label list without labels
        for t in (0.0, 0.25, float(np.nextafter(np.float32(0.5), np.float32(1))), float("nan")):
            assert call(rule=1, t=t) == 1 and b"0.5" in message()
        assert call(rule=0, t=float("nan")) == 1 and b"number" in message()
        assert call(capacity=-1) == 1 and b"index buffer" in message()
        assert call(indices=None) == 1 and b"index buffer" in message()
        for shape in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
            assert call(shape=shape) == 1 and b"positive" in message()
        for shape in ((1 << 11, 1 << 10, 1 << 10), (1 << 31, 1, 1), (1, 1 << 40, 1), (1 << 30, 1 << 30, 1 << 30)):
            assert call(shape=shape) == 1 and b"2^31" in message()
    assert lib.vgt_hip_cells_select(None, None, None, 0, 15, None, None, None, 0, 0, ctypes.byref(count)) == 1
    assert b"null" in lib.vgt_hip_last_error()
    assert lib.vgt_hip_cells_select(v, None, None, 0, 15, None, None, None, 0, 0, ctypes.byref(count)) == 1
    assert (values == 0.25).all() and (indices == -9).all() and (out_values == -9.0).all() and (out_labels == 9).all()
    assert count.value == -7
