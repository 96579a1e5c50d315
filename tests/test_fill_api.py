"""(not gpu) The enclosed-space entry points of the C ABI exist, are bound, and reject bad arguments before any HIP
call."""
import ctypes
import inspect
import os

import numpy as np
import pytest

from voxelized_geometry_tools_amd import capi, synthetic

NEW = ["vgt_hip_fill_enclosed", "vgt_hip_fill_enclosed_dev"]


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
    for name in ("fill_enclosed", "fill_enclosed_dev"):
        assert callable(getattr(capi.Context, name))
    solid = inspect.signature(capi.Context.mesh_sdf).parameters["solid"]
    assert solid.default is False                                          # today's results stay the default


def test_argument_errors_without_device(lib):
    """No context exists here (no device needed): every call must fail with code 1 and a message, touching nothing."""
    cells = np.full((4, 4, 4), 0.25, np.float32)
    count = ctypes.c_int64(-7)
    c = capi._ptr(cells)
    for fn in (lib.vgt_hip_fill_enclosed, lib.vgt_hip_fill_enclosed_dev):
        def call(ctx=c, cells=c, cb=4, shape=(4, 4, 4), uif=1):
            # (a non-null context pointer is never dereferenced before the other checks: the cells' address stands in)
            return fn(ctx, cells, cb, *shape, uif, ctypes.byref(count))

        def message():
            return lib.vgt_hip_last_error()

        assert call(ctx=None) == 1 and b"null" in message()
        assert call(cells=None) == 1 and b"null" in message()
        for cb in (0, 2, 12, 16, -4):
            assert call(cb=cb) == 1 and b"cell_bytes" in message()
        for shape in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
            assert call(shape=shape) == 1 and b"positive" in message()
        for shape in ((1 << 11, 1 << 10, 1 << 10), (1 << 31, 1, 1), (1, 1 << 40, 1), (1 << 30, 1 << 30, 1 << 30)):
            assert call(shape=shape) == 1 and b"2^31" in message()
    assert (cells == 0.25).all() and count.value == -7


def test_hollow_spheres_are_the_d1_spheres_without_their_interiors():
    shape = (64, 48, 56)
    solid = synthetic.occupancy_spheres(shape, seed=9)
    hollow = synthetic.hollow_spheres(shape, seed=9)
    assert hollow.dtype == np.float32 and set(np.unique(hollow)) == {0.0, 1.0}
    assert (hollow <= solid).all() and 0 < hollow.sum() < solid.sum()
    # every sphere's surface layer is still there: a cell of the solid grid with a free face neighbour stays filled
    free = solid == 0.0
    surface = np.zeros(shape, bool)
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        surface[tuple(lo)] |= free[tuple(hi)]
        surface[tuple(hi)] |= free[tuple(lo)]
    assert (hollow[surface & (solid == 1.0)] == 1.0).all()
