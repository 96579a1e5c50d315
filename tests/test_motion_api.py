"""(not gpu) vgt_hip_check_motions[_dev] and vgt_hip_motion_tile_samples: declared, bound and exported, the testing hook
by the testing library alone; the header holds the definition; every argument error that can be seen without a tree is
rejected with VGT_HIP_ERR_INVALID_ARGUMENT and its message before any device work (the ones that need a tree of the
context -- NULL joint arrays, E * J, a sphere's link, 641 links -- are in tests/test_gpu_motions.py); E == 0 succeeds
without a device; the tile sizes."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from voxelized_geometry_tools_amd import capi

NAMES = {"vgt_hip_check_motions": 28, "vgt_hip_check_motions_dev": 28, "vgt_hip_motion_tile_samples": 1}
HOOK = "vgt_hip_testing_set_motion_workgroups"


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
    assert hasattr(capi.Context, "check_motions") and hasattr(capi.Context, "check_motions_dev")
    assert hasattr(capi.Context, "set_motion_workgroups")
    assert capi.MotionChecks._fields == ("status", "first_collision", "min_clearance", "min_sample", "min_sphere",
                                         "min_gradient", "fk_status")


def test_header_holds_the_definition():
    text = open(os.path.join(ROOT, "include", "vgt_hip.h")).read()
    for needle in ("VGT_HIP_MOTION_STOP_AT_COLLISION 2u", "VGT_HIP_MOTION_CLEAR 0", "VGT_HIP_MOTION_COLLISION 1",
                   "VGT_HIP_MOTION_NO_VALUE 2", "VGT_HIP_MOTION_INVALID 3", "t = (double)k / (double)n",
                   "q_j = a_j + t * (b_j - a_j)", "q = a, the bits as given", "q = b, the bits as given",
                   "b is not read", "no wrap-around", "every bit of those seven values", "ties under == go to",
                   "the lowest k", "the OR of the considered samples' fk_status", "motion 12: num_steps -3",
                   "forms no address", "E == 0 succeeds without a device"):
        assert needle in text, needle
    assert (capi.MOTION_CLEAR, capi.MOTION_COLLISION, capi.MOTION_NO_VALUE, capi.MOTION_INVALID) == (0, 1, 2, 3)
    assert capi.MOTION_STOP_AT_COLLISION == 2 and capi.SPHERES_OUTSIDE_IS_COLLISION == 1


def test_argument_errors_and_empty_batch_without_device(lib):
    """No context and no tree exist here: non-null stand-ins are never dereferenced before the checks are through."""
    stand_in = np.zeros(64)
    p = capi._ptr(stand_in)
    status = np.full(4, 9, np.uint8)
    xyzr = np.tile([0.0, 0.0, 0.0, 0.1], (3, 1))
    link = np.zeros(3, np.int32)
    steps = np.array([2, 0, 5, 1], np.int32)
    for host, fn in ((True, lib.vgt_hip_check_motions), (False, lib.vgt_hip_check_motions_dev)):
        def call(ctx=p, sdf=p, shape=(4, 4, 4), res=0.1, xyzr=capi._ptr(xyzr), link=capi._ptr(link), s=3, tree=p,
                 a=p, b=p, steps=capi._ptr(steps), uniform=0, e=4, clearance=0.0, flags=0, st=capi._ptr(status)):
            return fn(ctx, sdf, *shape, res, None, None, xyzr, link, s, tree, a, b, steps, uniform, e, None, None,
                      clearance, flags, st, *([None] * 6))

        def refused(needle, **kw):
            rc = call(**kw)
            message = lib.vgt_hip_last_error()
            assert rc == 1 and needle in message, (kw, rc, message)

        for name in ("ctx", "sdf", "tree", "st", "xyzr", "link"):
            refused(b"null", **{name: None})
        for res in (0.0, -0.1, float("inf"), float("nan")):
            refused(b"resolution", res=res)
        refused(b"NaN", clearance=float("nan"))
        for flags in (4, 8, 0x80000000, 7):
            refused(b"unknown motion check flag", flags=flags)
        refused(b"negative", shape=(4, -1, 4))
        refused(b"negative", s=-1)
        refused(b"negative", e=-1)
        refused(b"uniform_steps -3 is negative", steps=None, uniform=-3)
        refused(b"2^31 cells", shape=(2048, 1024, 1024))
        refused(b"2^31 cells", shape=(2 ** 40, 2 ** 40, 2 ** 40))
        refused(b"2^31", e=2 ** 31)
        refused(b"2^31", s=2 ** 31)
        # nothing to do: success before the tree is looked at, with whatever is null that E == 0 does not need
        assert call(e=0) == 0
        assert call(e=0, a=None, b=None, steps=None, s=0, xyzr=None, link=None) == 0
        assert call(e=0, uniform=0, steps=None, flags=3) == 0
        # (a negative uniform_steps does not matter when num_steps is given)
        assert call(e=0, uniform=-3) == 0
        if host:
            # the host form looks at its arrays and names the first offender
            bad = steps.copy()
            bad[1], bad[3] = -3, -9
            refused(b"motion 1: num_steps -3", steps=capi._ptr(bad))
            for radius in (-0.5, float("nan")):
                model = xyzr.copy()
                model[1, 3] = model[2, 3] = radius
                refused(b"sphere 1: the radius must not be negative or NaN", xyzr=capi._ptr(model))
        # a tree that is not this context's (the stand-in's zeroed bytes name no context at all)
        refused(b"another context")
    assert (status == 9).all()


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
            ctx.check_motions(sdf, 0.1, xyzr, [0, 0], tree, np.zeros((3, 3)), np.zeros((3, 4)), 2)
        with pytest.raises(ValueError, match="same shape"):
            ctx.check_motions(sdf, 0.1, xyzr, [0, 0], tree, np.zeros((3, 4)), np.zeros((2, 4)), 2)
        with pytest.raises(ValueError, match="one count per motion"):
            ctx.check_motions(sdf, 0.1, xyzr, [0, 0], tree, np.zeros((3, 4)), np.zeros((3, 4)), [1, 2])
        with pytest.raises(ValueError, match="one link per sphere"):
            ctx.check_motions(sdf, 0.1, xyzr, [0], tree, np.zeros((3, 4)), np.zeros((3, 4)), 2)
        with pytest.raises(ValueError, match="motion 2: num_steps -1"):
            ctx.check_motions(sdf, 0.1, xyzr, [0, 0], tree, np.zeros((3, 4)), np.zeros((3, 4)), [1, 2, -1])
        got = ctx.check_motions(sdf, 0.1, xyzr, [0, 0], tree, np.zeros((0, 4)), np.zeros((0, 4)), 5)
    finally:
        tree.handle = None                                     # (nothing to destroy)
    assert got.status.shape == (0,) and got.min_gradient.shape == (0, 3) and got.first_collision.dtype == np.int32


def test_tile_samples(lib):
    """64 >= T(1) >= T(10) >= T(11) >= T(41) >= T(640) >= 1, powers of two, 96 L T <= 60 KiB; beyond 640 links: 0."""
    t = capi.motion_tile_samples
    assert 64 >= t(1) >= t(10) >= t(11) >= t(41) >= t(640) >= 1
    assert t(641) == 0 and t(0) == 0 and t(-1) == 0 and t(2 ** 40) == 0
    previous = 64
    for links in range(1, 641):
        tile = t(links)
        assert tile >= 1 and tile & (tile - 1) == 0 and 96 * links * tile <= 60 * 1024, links
        assert tile <= previous
        previous = tile
    assert t(640) == 1 and lib.vgt_hip_motion_tile_samples(8) == t(8)


def test_launch_geometry_hook(lib):
    """vgt_hip_testing_motion_launch_geometry: in the testing library only; its tile is vgt_hip_motion_tile_samples, the
    sphere table is in LDS for few spheres and not beyond some count that depends on the links, and what the launcher
    refuses the hook refuses."""
    name = "vgt_hip_testing_motion_launch_geometry"
    text = open(os.path.join(ROOT, "include", "vgt_hip.h")).read()
    testing_section = text[text.index("#ifdef VGT_HIP_TESTING"):text.index("#endif /* VGT_HIP_TESTING */")]
    assert name in testing_section and name in capi.TESTING_SIGNATURES and name not in capi.SIGNATURES
    assert hasattr(ctypes.CDLL(capi.TESTING_LIB_PATH), name) and not hasattr(ctypes.CDLL(capi.LIB_PATH), name)
    g = capi.motion_launch_geometry
    for links in (1, 8, 41, 640):
        assert g(links, 0).tile_samples == capi.motion_tile_samples(links)
        in_lds = [g(links, s).table_in_lds for s in range(0, 400)]
        assert in_lds[0] == 1 and in_lds[-1] == 0 and sorted(in_lds, reverse=True) == in_lds, links
    for links, spheres in ((641, 5), (0, 5), (8, -1)):
        with pytest.raises(ValueError):
            g(links, spheres)
    out = ctypes.c_int32(7)
    testing = capi.load(testing=True)
    assert testing.vgt_hip_testing_motion_launch_geometry(8, 5, None, ctypes.byref(out)) == 1 and out.value == 7
