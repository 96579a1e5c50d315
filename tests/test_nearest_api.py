"""(not gpu) The nearest-other-class entry points of include/vgt_hip.h: declared, bound and exported; every argument
error is rejected with VGT_HIP_ERR_INVALID_ARGUMENT and a message before any HIP call, outputs untouched; the workspace
holds 6 bytes per voxel plus hull stacks that grow with the axis lengths and not with the volume."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from voxelized_geometry_tools_amd import capi

NAMES = ("vgt_hip_nearest_workspace_bytes", "vgt_hip_nearest_dev", "vgt_hip_nearest_from_occupancy_f32",
         "vgt_hip_nearest_from_mask_u8", "vgt_hip_cells_nearest")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load()


def test_declared_bound_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "vgt_hip.h")).read()
    stripped = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(capi.LIB_PATH)
    testing = ctypes.CDLL(capi.TESTING_LIB_PATH)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, stripped), name
        assert name in capi.SIGNATURES
        assert hasattr(raw, name) and hasattr(testing, name), name
    assert lib.vgt_hip_abi_version() == 2
    # the contract is stated in the header: the border, the limits, the codes, the purity of the tie choice
    for needle in ("NO virtual border", "fewer than 2^31 cells", "0x7fffffff goes with", "pure function of the input"):
        assert needle in " ".join(text.split()), needle


def test_argument_errors_without_device(lib):
    """No context exists here (no device needed): every call must fail with code 1 and a message, touching nothing."""
    occ = np.zeros((4, 4, 4), np.float32)
    mask = np.zeros((4, 4, 4), np.uint8)
    nearest = np.full(64, 9, np.int32)
    d2 = np.full(64, 9, np.int32)
    ws = np.zeros(1 << 16, np.uint8)
    o, m, nr, d, w = (capi._ptr(a) for a in (occ, mask, nearest, d2, ws))

    def message():
        return lib.vgt_hip_last_error()

    # (a non-null context pointer is never dereferenced before the other checks: the grid's address stands in)
    def dev(ctx=o, occ=o, shape=(4, 4, 4), nearest=nr, d2=d, ws=w, ws_bytes=ws.size):
        return lib.vgt_hip_nearest_dev(ctx, occ, *shape, 1, nearest, d2, ws, ws_bytes)

    def host(ctx=o, occ=o, shape=(4, 4, 4), nearest=nr, d2=d):
        return lib.vgt_hip_nearest_from_occupancy_f32(ctx, occ, *shape, 1, nearest, d2)

    def from_mask(ctx=o, mask=m, shape=(4, 4, 4), nearest=nr, d2=d):
        return lib.vgt_hip_nearest_from_mask_u8(ctx, mask, *shape, nearest, d2)

    assert capi.nearest_workspace_bytes((4, 4, 4)) <= ws.size
    for call in (dev, host, from_mask):
        assert call(ctx=None) == 1 and b"null" in message()
        assert call(nearest=None) == 1 and b"null" in message()
        for shape in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
            assert call(shape=shape) == 1 and b"positive" in message()
        for shape in ((16385, 1, 1), (1, 16385, 1), (1, 1, 16385), (2 ** 40, 1, 1)):
            assert call(shape=shape) == 1 and b"16384" in message()
        for shape in ((2048, 1024, 1024), (16384, 16384, 8), (1291, 1291, 1291)):
            assert call(shape=shape) == 1 and b"2^31" in message()
    assert dev(occ=None) == 1 and b"null" in message()
    assert host(occ=None) == 1 and b"null" in message()
    assert from_mask(mask=None) == 1 and b"null" in message()
    assert dev(ws=None) == 1 and b"null" in message()
    need = capi.nearest_workspace_bytes((4, 4, 4))
    for ws_bytes in (0, 6 * 64, need - 1):
        assert dev(ws_bytes=ws_bytes) == 1 and b"workspace too small" in message()
    assert lib.vgt_hip_cells_nearest(None, None, None, 0, 1, nr, d, None) == 1 and b"null" in message()
    assert lib.vgt_hip_cells_nearest(o, None, None, 0, 1, nr, d, None) == 1 and b"null" in message()
    assert (nearest == 9).all() and (d2 == 9).all() and not ws.any()


def test_workspace_size(lib):
    assert capi.nearest_workspace_bytes((0, 4, 4)) == 0
    assert capi.nearest_workspace_bytes((4, 0, 4)) == 0
    assert capi.nearest_workspace_bytes((4, 4, 0)) == 0
    # over the limits: 0
    assert capi.nearest_workspace_bytes((16385, 1, 1)) == 0
    assert capi.nearest_workspace_bytes((2048, 1024, 1024)) == 0  # 2^31 cells
    for shape in ((1, 1, 1), (3, 2, 5), (70, 33, 130), (16384, 1, 1), (1, 1, 16384), (512, 512, 512)):
        assert capi.nearest_workspace_bytes(shape) >= 6 * int(np.prod(shape)), shape

    def beyond_the_records(shape):
        return capi.nearest_workspace_bytes(shape) - 6 * int(np.prod(shape))

    # The hull stacks: 8 bytes per row of a line and lane in flight, at most 131072 lanes and at most 1 GiB -- a bound
    # in the axis lengths alone (plus the alignment of the two record fields).
    def bound(shape):
        return 8 * max(shape[0], shape[1]) * 131072 + 512

    cube = beyond_the_records((1024, 1024, 1024))
    assert 0 < cube <= min(bound((1024, 1024, 1024)), 2 ** 30 + 512)
    # 2048 x 1024 x 1024 holds 2^31 cells, one more than the limit (its size is 0, above); the largest grid of that
    # shape within the limit has twice the cube's volume all the same, and the stacks do not follow it
    double = beyond_the_records((2047, 1024, 1024))
    assert 0 < double <= 2 ** 30 + 512 and double <= cube + 512
    # eight times the volume along z: the same axis lengths in x and y, the same stacks
    assert beyond_the_records((512, 512, 4096)) == beyond_the_records((512, 512, 512)) <= bound((512, 512, 512))
    # twice the x axis at the same volume: more
    assert beyond_the_records((1024, 512, 256)) > beyond_the_records((512, 512, 512))


def test_python_binding_refuses_before_a_device_is_needed(lib):
    class Stand(capi.Context):
        def __init__(self, lib, handle):
            self._lib, self.handle = lib, handle

        def close(self):
            pass

    occ = np.zeros((2, 2, 2), np.float32)
    ctx = Stand(lib, capi._ptr(occ))
    with pytest.raises(ValueError, match="nx, ny, nz"):
        ctx.nearest_from_occupancy(np.zeros((2, 2), np.float32))
    with pytest.raises(ValueError, match="nx, ny, nz"):
        ctx.nearest_from_mask(np.zeros(8, np.uint8))
    with pytest.raises(ValueError, match="positive"):
        ctx.nearest_from_occupancy(np.zeros((2, 0, 2), np.float32))
    with pytest.raises(ValueError, match="16384"):
        ctx.nearest_dev(1, (1, 16385, 1), 1, 1, 1 << 40)
    with pytest.raises(ValueError, match="workspace too small"):
        ctx.nearest_dev(1, (8, 8, 8), 1, 1, 6 * 512)
