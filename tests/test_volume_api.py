"""(not gpu) vgt_hip_rasterize_spheres[_dev] and vgt_hip_spheres_cover_points[_dev]: declared, bound and exported; the
header holds the pinned expressions; every argument error of include/vgt_hip.h is rejected with
VGT_HIP_ERR_INVALID_ARGUMENT and a message before any device work, outputs untouched, the host forms naming the first
bad sphere; the empty calls succeed without a device."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from voxelized_geometry_tools_amd import capi

GRID_NAMES = ("vgt_hip_rasterize_spheres", "vgt_hip_rasterize_spheres_dev")
POINT_NAMES = ("vgt_hip_spheres_cover_points", "vgt_hip_spheres_cover_points_dev")
HOOKS = ("vgt_hip_testing_set_sphere_volume_workgroups", "vgt_hip_testing_set_sphere_volume_counters")


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
    for name, arguments in [(n, 16) for n in GRID_NAMES] + [(n, 15) for n in POINT_NAMES]:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert name in capi.SIGNATURES and len(capi.SIGNATURES[name][1]) == arguments
        assert hasattr(raw, name) and hasattr(testing, name), name
    for hook in HOOKS:
        assert hook in capi.TESTING_SIGNATURES and hasattr(testing, hook) and not hasattr(raw, hook)
    assert lib.vgt_hip_abi_version() == 2
    for method in ("rasterize_spheres", "rasterize_spheres_dev", "spheres_cover_points", "spheres_cover_points_dev",
                   "set_sphere_volume_workgroups", "set_sphere_volume_counters"):
        assert callable(getattr(capi.Context, method))


def test_header_documents_the_calls():
    text = open(os.path.join(ROOT, "include", "vgt_hip.h")).read()
    for needle in ("VGT_HIP_SPHERES_KEEP 1u", "((m[r]*x + m[4+r]*y) + m[8+r]*z) + m[12+r]", "R         = radius + padding",
                   "((dx*dx + dy*dy) + dz*dz) <= R*R", "M[a]*w0 + M[4+a]*w1 + M[8+a]*w2 + M[12+a]",
                   "(i_a + 0.5) * resolution", "((T[r]*px + T[4+r]*py) + T[8+r]*pz) + T[12+r]", "x*ny*nz + y*nz + z",
                   "UNSIGNED minimum", "covers nothing", "forms no address", "quiet NaN"):
        assert needle in text, needle
    assert capi.SPHERES_KEEP == 1


class Arrays:
    def __init__(self, b=2, s=3, links=2, n=5, shape=(4, 4, 4)):
        self.xyzr = np.full((s, 4), 0.25)
        self.link = np.zeros(s, np.int32)
        self.poses = np.tile(np.eye(4).reshape(16), (b, links, 1))
        self.first = np.full(shape, 9, np.int32)
        self.points = np.full((n, 3), 0.5, np.float32)
        self.first_configuration = np.full(n, 9, np.int32)
        self.first_sphere = np.full(n, 9, np.int32)
        self.filtered = np.full((n, 3), 7.0, np.float32)

    def untouched(self):
        return ((self.first == 9).all() and (self.first_configuration == 9).all() and (self.first_sphere == 9).all()
                and (self.filtered == 7.0).all())


def message(lib):
    return lib.vgt_hip_last_error()


def shared_errors(lib, call):
    """The errors both forms share; call(**overrides) -> return code."""
    assert call(ctx=None) == 1 and b"null" in message(lib)
    assert call(xyzr=None) == 1 and b"null" in message(lib)
    assert call(link=None) == 1 and b"null" in message(lib)
    assert call(poses=None) == 1 and b"null" in message(lib)
    for counts in (dict(s=-1), dict(links=-1), dict(b=-1), dict(b=-(2 ** 40))):
        assert call(**counts) == 1 and b"negative" in message(lib)
    for padding in (math.nan, math.inf, -math.inf):
        assert call(padding=padding) == 1 and b"padding" in message(lib)
    assert call(links=0) == 1 and b"num_links == 0" in message(lib)
    # B * S >= 2^31 (the arrays are never looked at: the check comes first)
    assert call(s=2 ** 16, b=2 ** 15) == 1 and b"2^31" in message(lib) and b"pairs" in message(lib)
    assert call(s=2 ** 31, b=0) == 1 and b"2^31" in message(lib)
    assert call(links=2 ** 31) == 1 and b"2^31" in message(lib)
    assert call(b=2 ** 31, s=0) == 1 and b"2^31" in message(lib)


def test_grid_form_argument_errors_without_device(lib):
    """No context exists here (no device needed): every call must fail with code 1 and a message, touching nothing."""
    a = Arrays()
    xyzr, link, poses, first = (capi._ptr(x) for x in (a.xyzr, a.link, a.poses, a.first))
    for fn in (getattr(lib, name) for name in GRID_NAMES):
        # a non-null context pointer is never dereferenced before the other checks: the output's address stands in
        def call(ctx=first, shape=(4, 4, 4), res=0.1, xyzr=xyzr, link=link, s=3, poses=poses, links=2, b=2, padding=0.0,
                 base=0, flags=0, out=first):
            return fn(ctx, *shape, res, None, xyzr, link, s, poses, links, b, padding, base, flags, out)

        shared_errors(lib, call)
        assert call(out=None) == 1 and b"null" in message(lib)
        for shape in ((-1, 4, 4), (4, -4, 4), (4, 4, -(2 ** 40))):
            assert call(shape=shape) == 1 and b"negative" in message(lib)
        for shape in ((2048, 1024, 1024), (16384, 16384, 8), (1291, 1291, 1291), (2 ** 31, 1, 1), (2 ** 40, 2 ** 40, 2)):
            assert call(shape=shape) == 1 and b"2^31" in message(lib) and b"cells" in message(lib)
        for res in (0.0, -0.1, math.nan, math.inf, -math.inf):
            assert call(res=res) == 1 and b"resolution" in message(lib)
        for flags in (2, 3, 0x80000000):
            assert call(flags=flags) == 1 and b"flag" in message(lib)
        for base in (-1, 2 ** 31 - 2, 2 ** 31, 2 ** 40, -(2 ** 40)):             # base + 2 configurations > 2^31 - 1
            assert call(base=base) == 1 and b"first_configuration_base" in message(lib)
        # nothing to do: success before the (fake) context is touched -- an empty grid; for the device form also
        # nothing to lower in an array that is kept
        assert call(shape=(4, 0, 4)) == 0
        assert call(shape=(0, 0, 0), base=2 ** 31 - 3, flags=1) == 0
    assert lib.vgt_hip_rasterize_spheres_dev(first, 4, 4, 4, 0.1, None, xyzr, link, 3, None, 2, 0, 0.0, 0, 1, first) == 0
    assert lib.vgt_hip_rasterize_spheres_dev(first, 4, 4, 4, 0.1, None, None, None, 0, None, 0, 5, 0.0, 0, 1, first) == 0
    assert a.untouched()


def test_point_form_argument_errors_without_device(lib):
    a = Arrays()
    xyzr, link, poses, points = (capi._ptr(x) for x in (a.xyzr, a.link, a.poses, a.points))
    outs = [capi._ptr(x) for x in (a.first_configuration, a.first_sphere, a.filtered)]
    for fn in (getattr(lib, name) for name in POINT_NAMES):
        def call(ctx=points, points=points, n=5, xyzr=xyzr, link=link, s=3, poses=poses, links=2, b=2, padding=0.0,
                 flags=0, outs=outs):
            return fn(ctx, points, n, None, xyzr, link, s, poses, links, b, padding, flags, *outs)

        shared_errors(lib, call)
        assert call(points=None) == 1 and b"null" in message(lib)
        assert call(outs=[None, None, None]) == 1 and b"null" in message(lib)
        assert call(n=-1) == 1 and b"negative" in message(lib)
        assert call(n=2 ** 31) == 1 and b"2^31" in message(lib) and b"points" in message(lib)
        for flags in (1, 2, 0x80000000):
            assert call(flags=flags) == 1 and b"flag" in message(lib)
        # no points: success before the (fake) context is touched
        assert call(n=0) == 0
        assert call(n=0, points=None, b=0, poses=None) == 0
    assert a.untouched()


def test_the_host_forms_name_the_first_bad_sphere(lib):
    a = Arrays(s=5)
    first, points = capi._ptr(a.first), capi._ptr(a.points)
    outs = [capi._ptr(x) for x in (a.first_configuration, a.first_sphere, a.filtered)]

    def grid(xyzr, link):
        return lib.vgt_hip_rasterize_spheres(first, 4, 4, 4, 0.1, None, capi._ptr(xyzr), capi._ptr(link), 5,
                                             capi._ptr(a.poses), 2, 2, 0.0, 0, 0, first)

    def cloud(xyzr, link):
        return lib.vgt_hip_spheres_cover_points(points, points, 5, None, capi._ptr(xyzr), capi._ptr(link), 5,
                                                capi._ptr(a.poses), 2, 2, 0.0, 0, *outs)

    for call in (grid, cloud):
        for bad in (2, -1, 2 ** 31 - 1):
            link = a.link.copy()
            link[3] = bad
            link[4] = 7
            assert call(a.xyzr, link) == 1
            assert b"sphere 3: link %d" % bad in message(lib)
        for bad in (-0.5, math.nan, -math.inf):
            xyzr = a.xyzr.copy()
            xyzr[2, 3] = bad
            xyzr[4, 3] = -1.0
            assert call(xyzr, a.link) == 1
            assert b"sphere 2: the radius" in message(lib)
        # the first bad sphere, whatever is wrong with it
        xyzr, link = a.xyzr.copy(), a.link.copy()
        xyzr[1, 3] = -1.0
        link[0] = 5
        assert call(xyzr, link) == 1 and b"sphere 0:" in message(lib)
    assert a.untouched()


def test_nothing_to_cover_with_needs_no_device(lib):
    """B == 0 and S == 0 through the host forms: -1 everywhere (unless kept) and the plain copy, written on the host."""
    for s, b in ((0, 2), (3, 0), (0, 0)):
        a = Arrays(b=max(b, 1), s=max(s, 1))
        stand_in = capi._ptr(a.first)
        model = (capi._ptr(a.xyzr) if s else None, capi._ptr(a.link) if s else None, s, capi._ptr(a.poses) if b else None,
                 2, b)
        assert lib.vgt_hip_rasterize_spheres(stand_in, 4, 4, 4, 0.1, None, *model, 0.0, 0, 0, capi._ptr(a.first)) == 0
        assert (a.first == -1).all()
        a.first[1, 2, 3] = 5
        assert lib.vgt_hip_rasterize_spheres(stand_in, 4, 4, 4, 0.1, None, *model, 0.0, 7, 1, capi._ptr(a.first)) == 0
        assert a.first[1, 2, 3] == 5 and (a.first == -1).sum() == 63                   # kept as it was
        a.points[:] = np.arange(15, dtype=np.float32).reshape(5, 3)
        a.points[2] = [-0.0, np.nan, np.inf]
        assert lib.vgt_hip_spheres_cover_points(stand_in, capi._ptr(a.points), 5, None, *model, 0.0, 0,
                                                capi._ptr(a.first_configuration), capi._ptr(a.first_sphere),
                                                capi._ptr(a.filtered)) == 0
        assert (a.first_configuration == -1).all() and (a.first_sphere == -1).all()
        assert np.array_equal(a.filtered.view(np.uint32), a.points.view(np.uint32))
        # each output alone, and the copy onto the input itself
        c = Arrays()
        assert lib.vgt_hip_spheres_cover_points(stand_in, capi._ptr(a.points), 5, None, *model, 0.0, 0, None,
                                                capi._ptr(c.first_sphere), None) == 0
        assert (c.first_sphere == -1).all() and (c.first_configuration == 9).all() and (c.filtered == 7.0).all()
        before = a.points.copy()
        assert lib.vgt_hip_spheres_cover_points(stand_in, capi._ptr(a.points), 5, None, *model, 0.0, 0, None, None,
                                                capi._ptr(a.points)) == 0
        assert np.array_equal(a.points.view(np.uint32), before.view(np.uint32))


def test_python_binding_refuses_before_a_device_is_needed(lib):
    """Context.rasterize_spheres / spheres_cover_points pass the errors on as ValueError (through a stand-in context)."""
    class Stand(capi.Context):
        def __init__(self, lib, handle):
            self._lib, self.handle = lib, handle

        def close(self):
            pass

    anchor = np.zeros(4, np.float32)
    ctx = Stand(lib, capi._ptr(anchor))
    xyzr, link, poses = np.zeros((2, 4)), np.zeros(2, np.int32), np.zeros((3, 1, 16))
    points = np.zeros((4, 3), np.float32)
    with pytest.raises(ValueError, match="resolution"):
        ctx.rasterize_spheres((2, 2, 2), 0.0, xyzr, link, poses)
    with pytest.raises(ValueError, match="padding"):
        ctx.rasterize_spheres((2, 2, 2), 0.1, xyzr, link, poses, padding=math.nan)
    with pytest.raises(ValueError, match="first_configuration_base"):
        ctx.rasterize_spheres((2, 2, 2), 0.1, xyzr, link, poses, base=2 ** 31 - 3)
    with pytest.raises(ValueError, match="sphere 1: link"):
        ctx.rasterize_spheres((2, 2, 2), 0.1, xyzr, [0, 1], poses)
    with pytest.raises(ValueError, match="sphere 0: the radius"):
        ctx.spheres_cover_points(points, [[0, 0, 0, -1.0], [0, 0, 0, 1.0]], link, poses)
    with pytest.raises(ValueError, match="one link per sphere"):
        ctx.spheres_cover_points(points, xyzr, [0], poses)
    with pytest.raises(ValueError, match="shape"):
        ctx.rasterize_spheres((2, 2, 2), 0.1, xyzr, link, np.zeros((3, 1, 12)))
    with pytest.raises(ValueError, match="shape"):
        ctx.spheres_cover_points(points, xyzr, link, np.zeros((3, 1, 4, 3)))
    with pytest.raises(ValueError, match="into"):
        ctx.rasterize_spheres((2, 2, 2), 0.1, xyzr, link, poses, into=np.zeros((2, 2, 2), np.int64))
    with pytest.raises(ValueError, match="padding"):
        ctx.spheres_cover_points(points, xyzr, link, poses, padding=math.inf)
    first = ctx.rasterize_spheres((2, 3, 4), 0.1, xyzr, link, np.zeros((0, 1, 4, 4)))
    assert first.shape == (2, 3, 4) and first.dtype == np.int32 and (first == -1).all()
    kept = np.arange(24, dtype=np.int32).reshape(2, 3, 4)
    assert ctx.rasterize_spheres((2, 3, 4), 0.1, np.zeros((0, 4)), [], poses, base=5, into=kept) is kept
    assert np.array_equal(kept.reshape(-1), np.arange(24))
    got = ctx.spheres_cover_points(points, xyzr, link, np.zeros((0, 1, 16)), filtered=True)
    assert got.first_configuration.tolist() == [-1] * 4 and got.first_sphere.tolist() == [-1] * 4
    assert np.array_equal(got.filtered, points) and got.filtered is not points
    assert ctx.spheres_cover_points(points, xyzr, link, np.zeros((0, 1, 16))).filtered is None
    assert ctx.rasterize_spheres((0, 3, 4), 0.1, xyzr, link, poses).shape == (0, 3, 4)
