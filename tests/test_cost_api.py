"""(not gpu) vgt_hip_clearance_cost[_dev] and vgt_hip_cost_tile_samples: declared, bound and exported, the testing hook by
the testing library alone; the header holds the definition; every argument error that can be seen without a tree is
rejected with VGT_HIP_ERR_INVALID_ARGUMENT and its message before any device work (the ones that need a tree of the
context -- NULL joint values, B * J, B * L, a sphere's link, 513 links -- are in tests/test_gpu_cost.py); B == 0 succeeds
without a device; the tile sizes."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from voxelized_geometry_tools_amd import capi

NAMES = {"vgt_hip_clearance_cost": 24, "vgt_hip_clearance_cost_dev": 24, "vgt_hip_cost_tile_samples": 1}
HOOK = "vgt_hip_testing_set_cost_workgroups"


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return capi.load()


def test_declared_bound_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "vgt_hip.h")).read()
    testing_section = text[text.index("#ifdef VGT_HIP_TESTING"):text.index("#endif /* VGT_HIP_TESTING */")]
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    raw = ctypes.CDLL(capi.LIB_PATH)
    testing = ctypes.CDLL(capi.TESTING_LIB_PATH)
    for name, arguments in NAMES.items():
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in capi.SIGNATURES and len(capi.SIGNATURES[name][1]) == arguments
        assert hasattr(raw, name) and hasattr(testing, name), name
    assert HOOK in testing_section and HOOK not in capi.SIGNATURES
    assert HOOK in capi.TESTING_SIGNATURES and hasattr(testing, HOOK) and not hasattr(raw, HOOK)
    assert lib.vgt_hip_abi_version() == 2
    assert hasattr(capi.Context, "clearance_cost") and hasattr(capi.Context, "clearance_cost_dev")
    assert hasattr(capi.Context, "set_cost_workgroups")
    assert capi.ClearanceCosts._fields == ("cost", "joint_gradient", "num_active", "num_outside", "num_without_gradient",
                                           "fk_status")


def test_header_holds_the_definition():
    text = open(os.path.join(ROOT, "include", "vgt_hip.h")).read()
    for needle in ("c = (eps * 0.5) - d", "w = -1.0", "t = d - eps;  c = ((t * t) * 0.5) / eps", "w = t / eps",
                   "c = +0.0", "the comparisons in this order", "-0.0 < 0 is false",
                   "acc = +0.0; acc = acc + c_s for s ascending", "the summed form of vgt_hip_clearance_joint_gradient",
                   "is given weight 0 for the gradient; it still counts in cost", "spheres with a value and w != 0",
                   "spheres without a value", "nothing of either is restated here", "no output depends on the launch geometry",
                   "an unknown flag bit (any bit)", "forms no address", "B == 0 succeeds without a device",
                   "S == 0 gives cost +0.0, a gradient row of +0.0 and counts 0"):
        assert needle in text, needle


def test_argument_errors_and_empty_batch_without_device(lib):
    """No context and no tree exist here: non-null stand-ins are never dereferenced before the checks are through."""
    stand_in = np.zeros(64)
    p = capi._ptr(stand_in)
    cost = np.full(4, 9.0)
    others = [np.full((4, 3), 9.0), np.full(4, 9, np.int32), np.full(4, 9, np.int32), np.full(4, 9, np.int32),
              np.full(4, 9, np.uint8)]
    xyzr = np.tile([0.0, 0.0, 0.0, 0.1], (3, 1))
    link = np.zeros(3, np.int32)
    for host, fn in ((True, lib.vgt_hip_clearance_cost), (False, lib.vgt_hip_clearance_cost_dev)):
        def call(ctx=p, sdf=p, shape=(4, 4, 4), res=0.1, xyzr=capi._ptr(xyzr), link=capi._ptr(link), s=3, tree=p, q=p,
                 b=4, margin=0.25, flags=0, cost=capi._ptr(cost)):
            return fn(ctx, sdf, *shape, res, None, None, xyzr, link, s, tree, q, b, None, None, margin, flags, cost,
                      *[capi._ptr(o) for o in others])

        def refused(needle, **kw):
            rc = call(**kw)
            message = lib.vgt_hip_last_error()
            assert rc == 1 and needle in message, (kw, rc, message)

        for name in ("ctx", "sdf", "tree", "cost", "xyzr", "link"):
            refused(b"null", **{name: None})
        for res in (0.0, -0.1, float("inf"), float("nan")):
            refused(b"resolution", res=res)
        for margin in (0.0, -0.0, -0.25, float("inf"), float("-inf"), float("nan")):
            refused(b"margin must be positive and finite", margin=margin)
        for flags in (1, 2, 4, 0x80000000, 7):
            refused(b"unknown clearance cost flag", flags=flags)
        refused(b"negative", shape=(4, -1, 4))
        refused(b"negative", s=-1)
        refused(b"negative", b=-1)
        refused(b"2^31 cells", shape=(2048, 1024, 1024))
        refused(b"2^31 cells", shape=(2 ** 40, 2 ** 40, 2 ** 40))
        refused(b"2^31", b=2 ** 31)
        refused(b"2^31", s=2 ** 31)
        refused(b"(configuration, sphere) pairs", b=2 ** 30, s=2)
        refused(b"(configuration, sphere) pairs", b=(2 ** 31 + 2) // 3)          # the least such B for S = 3
        # nothing to do: success before the tree is looked at, with whatever is null that B == 0 does not need
        assert call(b=0) == 0
        assert call(b=0, q=None, s=0, xyzr=None, link=None) == 0
        if host:
            # the host form looks at the model and names the first offender
            for radius in (-0.5, float("nan")):
                model = xyzr.copy()
                model[1, 3] = model[2, 3] = radius
                refused(b"sphere 1: the radius must not be negative or NaN", xyzr=capi._ptr(model))
        # a tree that is not this context's (the stand-in's zeroed bytes name no context at all)
        refused(b"another context")
    assert (cost == 9.0).all()
    for o in others:
        assert (o == 9).all()


def test_python_binding_refuses_bad_shapes_before_the_library(lib):
    class Stand(capi.Context):
        def __init__(self, lib, handle):
            self._lib, self.handle = lib, handle

        def close(self):
            pass

    stand_in = np.zeros(64)
    ctx = Stand(lib, capi._ptr(stand_in))
    tree = capi.KinematicTree.__new__(capi.KinematicTree)
    tree.handle, tree.num_links, tree.num_joints, tree._lib = capi._ptr(stand_in), 6, 4, lib
    sdf, xyzr = np.zeros((4, 4, 4), np.float32), np.zeros((2, 4))
    try:
        with pytest.raises(ValueError, match=r"\[B, 4\]"):
            ctx.clearance_cost(sdf, 0.1, xyzr, [0, 0], tree, np.zeros((3, 3)), 0.25)
        with pytest.raises(ValueError, match="one link per sphere"):
            ctx.clearance_cost(sdf, 0.1, xyzr, [0], tree, np.zeros((3, 4)), 0.25)
        with pytest.raises(ValueError, match="margin must be positive and finite"):
            ctx.clearance_cost(sdf, 0.1, xyzr, [0, 0], tree, np.zeros((3, 4)), 0.0)
        got = ctx.clearance_cost(sdf, 0.1, xyzr, [0, 0], tree, np.zeros((0, 4)), 0.25)
        scored = ctx.clearance_cost(sdf, 0.1, xyzr, [0, 0], tree, np.zeros((0, 4)), 0.25, with_gradient=False)
    finally:
        tree.handle = None                                     # (nothing to destroy)
    assert got.cost.shape == (0,) and got.joint_gradient.shape == (0, 4) and got.num_active.dtype == np.int32
    assert scored.joint_gradient is None and scored.num_without_gradient is None and scored.fk_status.dtype == np.uint8


def test_tile_samples(lib):
    """64 >= T(1) >= T(2) >= ... >= T(512) = 1, powers of two, 96 L T <= 48 KiB; beyond 512 links: 0; a step of the tile
    size wherever 96 L T crosses the 6 KiB of the build."""
    t = capi.cost_tile_samples
    assert t(513) == 0 and t(0) == 0 and t(-1) == 0 and t(2 ** 40) == 0
    previous = 64
    steps = []
    for links in range(1, 513):
        tile = t(links)
        assert tile >= 1 and tile & (tile - 1) == 0 and 96 * links * tile <= 48 * 1024, links
        assert tile <= previous
        if tile < previous:
            steps.append(links)
        previous = tile
    assert t(1) == 64 and t(512) == 1 and lib.vgt_hip_cost_tile_samples(8) == t(8)
    # both sides of every step: the largest power of two whose poses fit 6 KiB
    assert steps == [2, 3, 5, 9, 17, 33]
    for links in steps:
        assert t(links - 1) == 2 * t(links) and 96 * (links - 1) * t(links - 1) <= 6 * 1024 < 96 * links * t(links - 1)


def test_launch_geometry_hook(lib):
    """vgt_hip_testing_cost_launch_geometry: in the testing library only; its tile is vgt_hip_cost_tile_samples, the passes
    are a power of two within the tile, the cost-only form has no links in LDS, few links and spheres sit in LDS and many
    do not, and what the launcher refuses the hook refuses."""
    name = "vgt_hip_testing_cost_launch_geometry"
    text = open(os.path.join(ROOT, "include", "vgt_hip.h")).read()
    testing_section = text[text.index("#ifdef VGT_HIP_TESTING"):text.index("#endif /* VGT_HIP_TESTING */")]
    assert name in testing_section and name in capi.TESTING_SIGNATURES and name not in capi.SIGNATURES
    assert hasattr(ctypes.CDLL(capi.TESTING_LIB_PATH), name) and not hasattr(ctypes.CDLL(capi.LIB_PATH), name)
    g = capi.cost_launch_geometry
    for links in (1, 8, 33, 463, 512):
        for spheres in (0, 1, 5, 64, 65, 257):
            for gradient in (True, False):
                got = g(links, spheres, gradient)
                assert got.tile_samples == capi.cost_tile_samples(links)
                assert got.passes >= 1 and got.passes & (got.passes - 1) == 0 and got.passes <= max(got.tile_samples, 1)
                assert gradient or not got.links_in_lds
                assert spheres <= 256 or not got.table_in_lds
    assert g(8, 21, True) == (capi.cost_tile_samples(8), g(8, 21, True).passes, 1, 1)
    assert g(512, 5, True).links_in_lds == 0
    for links, spheres in ((513, 5), (0, 5), (8, -1)):
        with pytest.raises(ValueError):
            g(links, spheres)
    out = [ctypes.c_int32(7) for _ in range(3)]
    testing = capi.load(testing=True)
    rc = testing.vgt_hip_testing_cost_launch_geometry(8, 5, 1, None, *[ctypes.byref(o) for o in out])
    assert rc == 1 and [o.value for o in out] == [7, 7, 7]
