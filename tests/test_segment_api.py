"""(not gpu) vgt_hip_cast_segments[_dev]: declared, bound and exported; every argument error of include/vgt_hip.h is
rejected with VGT_HIP_ERR_INVALID_ARGUMENT and a message before any device work, outputs untouched; an empty batch and
an empty grid succeed and touch nothing."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from voxelized_geometry_tools_amd import capi

NAMES = ("vgt_hip_cast_segments", "vgt_hip_cast_segments_dev")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load()


def test_declared_bound_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "vgt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(capi.LIB_PATH)
    testing = ctypes.CDLL(capi.TESTING_LIB_PATH)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in capi.SIGNATURES and len(capi.SIGNATURES[name][1]) == 19
        assert hasattr(raw, name) and hasattr(testing, name), name
    assert lib.vgt_hip_abi_version() == 2


def test_header_documents_the_call():
    text = open(os.path.join(ROOT, "include", "vgt_hip.h")).read()
    for needle in ("VGT_HIP_SEGMENT_OCCUPANCY 0", "VGT_HIP_SEGMENT_SDF_BELOW 1", "VGT_HIP_SEGMENT_WALK_THROUGH 1u",
                   "VGT_HIP_SEGMENT_CLEAR 0", "VGT_HIP_SEGMENT_HIT 1", "VGT_HIP_SEGMENT_MISSED_GRID 2",
                   "VGT_HIP_SEGMENT_INVALID 3", "tmin + 1e-10 > length", "((m0*x + m4*y) + m8*z) + m12"):
        assert needle in text, needle
    assert (capi.SEGMENT_OCCUPANCY, capi.SEGMENT_SDF_BELOW, capi.SEGMENT_WALK_THROUGH) == (0, 1, 1)
    assert (capi.SEGMENT_CLEAR, capi.SEGMENT_HIT, capi.SEGMENT_MISSED_GRID, capi.SEGMENT_INVALID) == (0, 1, 2, 3)


def test_argument_errors_without_device(lib):
    """No context exists here (no device needed): every call must fail with code 1 and a message, touching nothing."""
    field = np.zeros((4, 4, 4), np.float32)
    segments = np.full((2, 6), 0.2)
    status = np.full(2, 9, np.uint8)
    hit_index = np.full(2, 9, np.int32)
    fraction = np.full(2, 7.0)
    examined = np.full(2, 9, np.int32)
    min_value = np.full(2, 7.0, np.float32)
    min_index = np.full(2, 9, np.int32)
    f, s, st, hi, fr, ex, mv, mi = (capi._ptr(a) for a in (field, segments, status, hit_index, fraction, examined,
                                                           min_value, min_index))
    for fn in (getattr(lib, name) for name in NAMES):
        # a non-null context pointer is never dereferenced before the other checks: the field's address stands in
        def call(ctx=f, field=f, shape=(4, 4, 4), res=0.1, mode=1, threshold=0.0, flags=0, s=s, n=2, st=st, mv=mv, mi=mi):
            return fn(ctx, field, *shape, res, mode, 1, threshold, flags, None, s, n, st, hi, fr, ex, mv, mi)

        def message():
            return lib.vgt_hip_last_error()

        assert call(ctx=None) == 1 and b"null" in message()
        assert call(field=None) == 1 and b"null" in message()
        assert call(s=None) == 1 and b"null" in message()
        assert call(st=None) == 1 and b"null" in message()
        assert call(n=-1) == 1 and b"null" in message()
        for shape in ((-1, 4, 4), (4, -4, 4), (4, 4, -(2 ** 40))):
            assert call(shape=shape) == 1 and b"negative" in message()
        for shape in ((2048, 1024, 1024), (16384, 16384, 8), (1291, 1291, 1291), (2 ** 31, 1, 1), (2 ** 40, 2 ** 40, 2)):
            assert call(shape=shape) == 1 and b"2^31" in message()
        for res in (0.0, -0.1, math.nan, math.inf, -math.inf):
            assert call(res=res) == 1 and b"resolution" in message()
        for mode in (-1, 2, 7):
            assert call(mode=mode) == 1 and b"mode" in message()
        for flags in (2, 3, 0x80000000):
            assert call(flags=flags) == 1 and b"flag" in message()
        assert call(threshold=math.nan) == 1 and b"threshold" in message()
        # occupancy mode: the threshold is not looked at, the min outputs are refused one by one
        assert call(mode=0, mi=None) == 1 and b"min_value" in message()
        assert call(mode=0, mv=None) == 1 and b"min_value" in message()
        # nothing to do: success, before the (fake) context is touched
        assert call(n=0) == 0
        assert call(n=0, s=None) == 0
        assert call(shape=(4, 0, 4)) == 0
        assert call(mode=0, threshold=math.nan, mv=None, mi=None, n=0) == 0
        assert call(threshold=math.inf, flags=1, n=0) == 0
    assert (status == 9).all() and (hit_index == 9).all() and (fraction == 7.0).all() and (examined == 9).all()
    assert (min_value == 7.0).all() and (min_index == 9).all()


def test_python_binding_refuses_before_a_device_is_needed(lib):
    """Context.cast_segments passes the errors on as ValueError (no context can be made here, so through a stand-in)."""
    class Stand(capi.Context):
        def __init__(self, lib, handle):
            self._lib, self.handle = lib, handle

        def close(self):
            pass

    field = np.zeros((2, 2, 2), np.float32)
    ctx = Stand(lib, capi._ptr(field))
    with pytest.raises(ValueError, match="resolution"):
        ctx.cast_segments(field, 0.0, np.zeros((1, 6)))
    with pytest.raises(ValueError, match="mode"):
        ctx.cast_segments(field, 0.1, np.zeros((1, 6)), mode=5)
    with pytest.raises(ValueError, match="min_value"):
        ctx.cast_segments(field, 0.1, np.zeros((1, 6)), with_min=True)
    with pytest.raises(ValueError, match="threshold"):
        ctx.cast_segments(field, 0.1, np.zeros((1, 6)), mode=capi.SEGMENT_SDF_BELOW, threshold=math.nan)
    got = ctx.cast_segments(field, 0.1, np.zeros((0, 6)), mode=capi.SEGMENT_SDF_BELOW, with_min=True)
    assert [a.shape for a in got] == [(0,)] * 6 and got.status.dtype == np.uint8 and got.min_value.dtype == np.float32
