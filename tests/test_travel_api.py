"""(not gpu) The travel-cost and path-tracing entry points of the C ABI exist, are bound, and reject bad arguments before
any HIP call, through the product library."""
import ctypes
import os

import numpy as np
import pytest

from voxelized_geometry_tools_amd import capi

NEW = ["vgt_hip_travel_cost_workspace_bytes", "vgt_hip_travel_cost", "vgt_hip_travel_cost_dev",
       "vgt_hip_cells_travel_cost", "vgt_hip_trace_paths", "vgt_hip_trace_paths_dev"]


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
    for name in ("travel_cost", "travel_cost_dev", "trace_paths", "trace_paths_dev"):
        assert callable(getattr(capi.Context, name))
    assert callable(capi.Cells.travel_cost)
    header = open(os.path.join(os.path.dirname(capi.__file__), "..", "include", "vgt_hip.h")).read()
    for name in NEW:
        assert header.count(name + "(") == 1
    for name, value in (("TRAVEL_OCCUPANCY", "0"), ("TRAVEL_SDF_ABOVE", "1"), ("TRAVEL_NO_CORNER_CUTTING", "1u"),
                        ("TRAVEL_UNREACHED", "0xffffffffu"), ("TRACE_OK", "0"), ("TRACE_UNREACHED", "1"),
                        ("TRACE_TRUNCATED", "2"), ("TRACE_INVALID", "3")):
        assert "#define VGT_HIP_%s %s\n" % (name, value) in header
        assert getattr(capi, name) == int(value.rstrip("u"), 0)


def test_workspace_size(lib):
    for shape in ((0, 4, 4), (4, 0, 4), (4, 4, 0), (-1, 4, 4), (1 << 11, 1 << 10, 1 << 10), (1 << 31, 1, 1),
                  (1, 1 << 40, 1), (1 << 30, 1 << 30, 1 << 30)):
        assert capi.travel_cost_workspace_bytes(shape) == 0, shape
    # 32 bytes of status, two 4-byte flags per tile of 8 x 8 x 16 cells, 1 bit per cell; 256-byte aligned pieces
    assert capi.travel_cost_workspace_bytes((1, 1, 1)) == 4 * 256
    tiles = 3 * 2 * 3
    assert capi.travel_cost_workspace_bytes((17, 10, 33)) == 256 + 2 * 256 + (17 * 10 * 33 + 63) // 64 * 8 // 256 * 256 + 256
    assert tiles * 4 <= 256
    n = 256 ** 3
    assert capi.travel_cost_workspace_bytes((256, 256, 256)) == 256 + 2 * (32 * 32 * 16 * 4) + n // 8


def test_travel_cost_argument_errors_without_device(lib):
    """No context exists here (no device needed): every call must fail with code 1 and a message, touching nothing."""
    field = np.full((4, 4, 4), 0.25, np.float32)
    good_weights = np.array([10, 14, 17], np.uint32)
    sources = np.zeros(2, np.int32)
    cost = np.full((4, 4, 4), 7, np.uint32)
    toward = np.full((4, 4, 4), 7, np.int32)
    reached = ctypes.c_int64(-7)
    v = capi._ptr(field)
    workspace = np.zeros(4096, np.uint8)

    def message():
        return lib.vgt_hip_last_error()

    for dev in (False, True):
        def call(ctx=v, fld=v, shape=(4, 4, 4), mode=0, threshold=0.0, weights=good_weights, flags=0, src=sources,
                 num_sources=2, limit=capi.TRAVEL_NO_LIMIT, out=cost, ws=workspace, ws_bytes=4096):
            # (a non-null context pointer is never dereferenced before the other checks: the field's address stands in)
            args = [ctx, fld, *shape, mode, 1, threshold, capi._ptr(weights), flags, capi._ptr(src), None, num_sources,
                    limit, capi._ptr(out), capi._ptr(toward), ctypes.byref(reached)]
            if dev:
                return lib.vgt_hip_travel_cost_dev(*args, capi._ptr(ws), ws_bytes)
            return lib.vgt_hip_travel_cost(*args)

        assert call(ctx=None) == 1 and b"null" in message()
        assert call(fld=None) == 1 and b"null" in message()
        assert call(weights=None) == 1 and b"null" in message()
        assert call(out=None) == 1 and b"null" in message()
        assert call(src=None) == 1 and b"null" in message()
        assert call(num_sources=-1) == 1 and b"negative" in message()
        for shape in ((4, -1, 4), (-4, 4, 4), (4, 4, -1)):
            assert call(shape=shape) == 1 and b"negative" in message()
        for shape in ((1 << 11, 1 << 10, 1 << 10), (1 << 31, 1, 1), (1, 1 << 40, 1), (1 << 30, 1 << 30, 1 << 30)):
            assert call(shape=shape) == 1 and b"2^31" in message()
        for mode in (2, -1, 7):
            assert call(mode=mode) == 1 and b"mode" in message()
        for flags in (2, 3, 0x80000000):
            assert call(flags=flags) == 1 and b"flag" in message()
        assert call(mode=1, threshold=float("nan")) == 1 and b"threshold" in message()
        assert call(weights=np.array([0, 14, 17], np.uint32)) == 1 and b"weights[0]" in message()
        for bad in ([65536, 0, 0], [1, 65536, 0], [1, 0, 1 << 31]):
            assert call(weights=np.array(bad, np.uint32)) == 1 and b"65535" in message()
        assert call(limit=0xffffffff) == 1 and b"limit" in message()
        if dev:
            need = capi.travel_cost_workspace_bytes((4, 4, 4))
            assert call(ws=None) == 1 and b"null" in message()
            assert call(ws_bytes=need - 1) == 1 and b"workspace" in message()
        # an empty grid succeeds before the context is looked into, and writes nothing but the count
        for shape in ((0, 4, 4), (4, 0, 4), (4, 4, 0)):
            reached.value = -7
            assert call(shape=shape, ws=None, ws_bytes=0) == 0 and reached.value == 0
        reached.value = -7

    assert lib.vgt_hip_cells_travel_cost(None, v, None, 0, 1, capi._ptr(good_weights), 0, capi._ptr(sources), None, 2,
                                         capi.TRAVEL_NO_LIMIT, capi._ptr(cost), None, None) == 1 and b"null" in message()
    assert lib.vgt_hip_cells_travel_cost(v, None, None, 0, 1, capi._ptr(good_weights), 0, capi._ptr(sources), None, 2,
                                         capi.TRAVEL_NO_LIMIT, capi._ptr(cost), None, None) == 1 and b"null" in message()
    assert reached.value == -7 and (cost == 7).all() and (toward == 7).all()


def test_trace_argument_errors_without_device(lib):
    toward = np.zeros(8, np.int32)
    starts = np.zeros(3, np.int32)
    paths = np.full((3, 4), 7, np.int32)
    lengths = np.full(3, 7, np.int32)
    status = np.full(3, 7, np.uint8)
    v = capi._ptr(toward)
    for fn in (lib.vgt_hip_trace_paths, lib.vgt_hip_trace_paths_dev):
        def call(ctx=v, tw=toward, cells=8, st=starts, num=3, max_cells=4, p=paths, ln=lengths, s=status):
            return fn(ctx, capi._ptr(tw), cells, capi._ptr(st), num, max_cells, capi._ptr(p), capi._ptr(ln), capi._ptr(s))

        def message():
            return lib.vgt_hip_last_error()

        assert call(ctx=None) == 1 and b"null" in message()
        assert call(tw=None) == 1 and b"null" in message()
        assert call(st=None) == 1 and b"null" in message()
        assert call(p=None) == 1 and call(ln=None) == 1 and call(s=None) == 1
        assert call(num=-1) == 1 and b"negative" in message()
        assert call(cells=-1) == 1 and call(cells=1 << 31) == 1 and b"2^31" in message()
        for max_cells in (0, -1):
            assert call(max_cells=max_cells) == 1 and b"max_cells" in message()
        assert call(num=0, st=None) == 0          # nothing to trace: success before the context is looked into
    assert (paths == 7).all() and (lengths == 7).all() and (status == 7).all()
