"""(not gpu) The mesh entry points of the C ABI exist, are bound, reject bad arguments before any HIP call, and
vgt_hip_mesh_grid_for (pure host code) equals the restatement bit for bit."""
import ctypes
import math
import os

import numpy as np
import pytest

import mesh_ref as M
from test_mesh_ref import SLANTED, independent_meshes
from voxelized_geometry_tools_amd import capi, synthetic

NEW = ["vgt_hip_rasterize_mesh", "vgt_hip_rasterize_mesh_dev", "vgt_hip_mesh_grid_for"]


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
    for name in ("rasterize_mesh", "rasterize_mesh_dev", "mesh_sdf"):
        assert callable(getattr(capi.Context, name))
    assert callable(capi.mesh_grid_for) and (capi.MESH_RULE_REFERENCE, capi.MESH_RULE_NEAREST) == (0, 1)


def test_argument_errors_without_device(lib):
    """No context exists here (no device needed): every call must fail with code 1 and a message, touching nothing."""
    vertices = np.array([[0.1, 0.1, 0.1], [0.3, 0.1, 0.1], [0.1, 0.3, 0.1]])
    triangles = np.array([[0, 1, 2]], np.int32)
    cells = np.zeros((4, 4, 4), np.float32)
    xf = np.eye(4).reshape(16)
    v, t, c, m = (capi._ptr(a) for a in (vertices, triangles, cells, xf))
    fake_ctx = ctypes.c_void_p(0)
    for fn in (lib.vgt_hip_rasterize_mesh, lib.vgt_hip_rasterize_mesh_dev):
        def call(ctx=fake_ctx, v=v, nv=3, t=t, nt=1, c=c, cb=4, shape=(4, 4, 4), res=0.1, wfg=None, gfw=None, rule=0):
            return fn(ctx, v, nv, t, nt, c, cb, *shape, res, wfg, gfw, 0, rule)

        def message():
            return lib.vgt_hip_last_error()

        assert call() == 1 and b"null" in message()                       # (no context)
        # a non-null context pointer is never dereferenced before the other checks: use the cells' address as a stand-in
        ctx = c
        assert call(ctx, v=None) == 1 and b"null" in message()
        assert call(ctx, t=None) == 1 and b"null" in message()
        assert call(ctx, c=None) == 1 and b"null" in message()
        for shape in ((0, 4, 4), (4, -1, 4), (4, 4, 0)):
            assert call(ctx, shape=shape) == 1 and b"positive" in message()
        assert call(ctx, shape=(1 << 30, 1 << 30, 1 << 30)) == 1 and b"2^40" in message()
        for res in (0.0, -0.1, math.nan, math.inf):
            assert call(ctx, res=res) == 1 and b"resolution" in message()
        for cb in (0, 2, 12, 16):
            assert call(ctx, cb=cb) == 1 and b"cell_bytes" in message()
        for rule in (-1, 2):
            assert call(ctx, rule=rule) == 1 and b"rule" in message()
        assert call(ctx, nv=-1) == 1 and b"negative" in message()
        assert call(ctx, nt=-1) == 1 and b"negative" in message()
        assert call(ctx, wfg=m) == 1 and b"both transforms" in message()
        assert call(ctx, gfw=m) == 1 and b"both transforms" in message()
    assert not cells.any()

    counts = (ctypes.c_int64 * 3)(7, 7, 7)
    origin = np.full(3, 7.0)
    n = [ctypes.byref(counts, 8 * a) for a in range(3)]
    o = capi._ptr(origin)
    grid_for = lib.vgt_hip_mesh_grid_for
    assert grid_for(None, 3, 0.1, *n, o) == 1 and b"null" in lib.vgt_hip_last_error()
    assert grid_for(v, 3, 0.1, None, n[1], n[2], o) == 1 and b"null" in lib.vgt_hip_last_error()
    assert grid_for(v, 3, 0.1, *n, None) == 1 and b"null" in lib.vgt_hip_last_error()
    assert grid_for(v, 0, 0.1, *n, o) == 1 and b"vertex" in lib.vgt_hip_last_error()
    assert grid_for(v, -2, 0.1, *n, o) == 1
    for res in (0.0, -1.0, math.nan, math.inf):
        assert grid_for(v, 3, res, *n, o) == 1 and b"resolution" in lib.vgt_hip_last_error()
    bad = vertices.copy()
    bad[1, 2] = math.nan
    assert grid_for(capi._ptr(bad), 3, 0.1, *n, o) == 1 and b"finite" in lib.vgt_hip_last_error()
    assert grid_for(v, 3, 1e-12, *n, o) == 1 and b"2^31" in lib.vgt_hip_last_error()
    assert list(counts) == [7, 7, 7] and (origin == 7.0).all()


def test_mesh_grid_for_equals_the_restatement(lib):
    cases = [(SLANTED, 0.125), (SLANTED + 3.0, 0.03), (np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), 0.125),
             (synthetic.mesh_torus()[0], 0.04), (synthetic.mesh_box((-0.3, 0.1, 0.2), (0.9, 0.7, 1.3))[0], 0.1)]
    cases += [(v, res) for _, v, _, res in independent_meshes()]
    for vertices, res in cases:
        shape, origin = capi.mesh_grid_for(vertices, res)
        want_shape, want_origin = M.mesh_grid_for(vertices, res)
        assert shape == want_shape
        assert origin.dtype == np.float64 and np.array_equal(origin.view(np.uint64), want_origin.view(np.uint64))
