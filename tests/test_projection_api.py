"""(not gpu) Argument checks of vgt_hip_sdf_project_out_of_collision[_dev]: each is rejected with
VGT_HIP_ERR_INVALID_ARGUMENT and a message before any device work, outputs untouched."""
import math
import os

import numpy as np
import pytest

from voxelized_geometry_tools_amd import capi


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load()


def test_argument_errors_without_device(lib):
    """No context exists here (no device needed): every call must fail with code 1 and a message, touching nothing."""
    sdf = np.zeros((4, 4, 4), np.float32)
    queries = np.full((2, 3), 0.2)
    position = np.full((2, 3), 7.0)
    has = np.full(2, 9, np.uint8)
    status = np.full(2, 9, np.uint8)
    iterations = np.full(2, 9, np.int32)
    s, q, p, h, st, it = (capi._ptr(a) for a in (sdf, queries, position, has, status, iterations))
    for fn in (lib.vgt_hip_sdf_project_out_of_collision, lib.vgt_hip_sdf_project_out_of_collision_dev):
        # a non-null context pointer is never dereferenced before the other checks: the field's address stands in
        def call(ctx=s, field=s, shape=(4, 4, 4), res=0.1, q=q, n=2, clearance=0.0, multiplier=0.1, limit=0, p=p):
            return fn(ctx, field, *shape, res, None, None, q, n, clearance, multiplier, limit, p, h, st, it)

        def message():
            return lib.vgt_hip_last_error()

        assert call(ctx=None) == 1 and b"null" in message()
        assert call(field=None) == 1 and b"null" in message()
        assert call(q=None) == 1 and b"null" in message()
        assert call(p=None) == 1 and b"null" in message()
        assert call(n=-1) == 1 and b"null" in message()
        for shape in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
            assert call(shape=shape) == 1 and b"positive" in message()
        for shape in ((2048, 1024, 1024), (16384, 16384, 8), (1291, 1291, 1291)):
            assert call(shape=shape) == 1 and b"2^31" in message()
        for res in (0.0, -0.1, math.nan, math.inf):
            assert call(res=res) == 1 and b"resolution" in message()
        for multiplier in (0.0, -0.1, math.nan, math.inf, -math.inf):
            assert call(multiplier=multiplier) == 1 and b"stepsize_multiplier" in message()
        assert call(clearance=math.nan) == 1 and b"minimum_distance" in message()
        for limit in (-1, -(2 ** 31)):
            assert call(limit=limit) == 1 and b"max_iterations" in message()
    assert (position == 7.0).all() and (has == 9).all() and (status == 9).all() and (iterations == 9).all()


def test_header_documents_the_call():
    from conftest import ROOT
    text = open(os.path.join(ROOT, "include", "vgt_hip.h")).read()
    for needle in ("VGT_HIP_PROJECT_OK 0", "VGT_HIP_PROJECT_OUTSIDE 1", "VGT_HIP_PROJECT_FLAT_GRADIENT 2",
                   "VGT_HIP_PROJECT_LEFT_GRID 3", "VGT_HIP_PROJECT_ITERATION_LIMIT 4",
                   "norm = sqrt((gx*gx + gy*gy) + gz*gz)"):
        assert needle in text, needle
    assert (capi.PROJECT_OK, capi.PROJECT_OUTSIDE, capi.PROJECT_FLAT_GRADIENT, capi.PROJECT_LEFT_GRID,
            capi.PROJECT_ITERATION_LIMIT) == (0, 1, 2, 3, 4)
