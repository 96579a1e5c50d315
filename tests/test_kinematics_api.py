"""(not gpu) vgt_hip_kinematics_create / _destroy, vgt_hip_forward_kinematics[_dev] and
vgt_hip_clearance_joint_gradient[_dev]: declared, bound and exported; every argument error of include/vgt_hip.h is
rejected with VGT_HIP_ERR_INVALID_ARGUMENT and a message before any device work, a bad tree naming its first offending
link; B == 0 succeeds without a device; what can be said about a handle's life without one."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from voxelized_geometry_tools_amd import capi

NAMES = {"vgt_hip_kinematics_create": 9, "vgt_hip_kinematics_destroy": 1, "vgt_hip_kinematics_num_links": 1,
         "vgt_hip_kinematics_num_joints": 1, "vgt_hip_kinematics_lds_links": 0, "vgt_hip_forward_kinematics": 8,
         "vgt_hip_forward_kinematics_dev": 8, "vgt_hip_clearance_joint_gradient": 12,
         "vgt_hip_clearance_joint_gradient_dev": 12, "vgt_hip_check_spheres_from_joints": 28}
HOOK = "vgt_hip_testing_set_kinematics_workgroups"


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
    for name, arguments in NAMES.items():
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in capi.SIGNATURES and len(capi.SIGNATURES[name][1]) == arguments
        assert hasattr(raw, name) and hasattr(testing, name), name
    assert HOOK in capi.TESTING_SIGNATURES and hasattr(testing, HOOK) and not hasattr(raw, HOOK)
    assert 1 <= lib.vgt_hip_kinematics_lds_links() == capi.kinematics_lds_links() <= 10   # (64 KiB / 6 KiB per link)


def test_header_documents_the_calls():
    text = open(os.path.join(ROOT, "include", "vgt_hip.h")).read()
    for needle in ("VGT_HIP_JOINT_FIXED 0", "VGT_HIP_JOINT_REVOLUTE 1", "VGT_HIP_JOINT_PRISMATIC 2",
                   "VGT_HIP_FK_NOT_COMPUTABLE 1", "VGT_HIP_FK_OUTSIDE_LIMITS 2", "0x1.45f306dc9c883p-1",
                   "0x1.921fb54400000p+0", "0x1.0b4611a600000p-34", "0x1.3198a2e037073p-69", "sin_r = r + (r*z)*ps",
                   "cos_r = 1 + z*pc", "R01 = (x*y)*v - z*s", "(A_r0*B_0c + A_r1*B_1c) + A_r2*B_2c",
                   "term = (g0*u0 + g1*u1) + g2*u2", "acc_j = acc_j + w*term"):
        assert needle in text, needle
    assert (capi.JOINT_FIXED, capi.JOINT_REVOLUTE, capi.JOINT_PRISMATIC) == (0, 1, 2)
    assert (capi.FK_NOT_COMPUTABLE, capi.FK_OUTSIDE_LIMITS) == (1, 2)


class TreeArrays:
    def __init__(self, links=6, joints=4):
        self.links, self.joints = links, joints
        self.parent = np.arange(-1, links - 1, dtype=np.int32)
        self.joint_type = np.array([1, 2, 0, 1, 1, 2][:links], np.int32)
        self.joint_index = np.array([0, 1, 0, 2, 3, 3][:links], np.int32)
        self.axis = np.tile([0.0, 0.0, 1.0], (links, 1))
        self.origin = np.tile(np.eye(4).reshape(16), (links, 1))

    def create(self, lib, ctx, out, **kw):
        a = dict(links=self.links, joints=self.joints, parent=capi._ptr(self.parent),
                 joint_type=capi._ptr(self.joint_type), joint_index=capi._ptr(self.joint_index),
                 axis=capi._ptr(self.axis), origin=capi._ptr(self.origin))
        a.update(kw)
        return lib.vgt_hip_kinematics_create(ctx, a["links"], a["joints"], a["parent"], a["joint_type"],
                                             a["joint_index"], a["axis"], a["origin"], out)


def test_create_refuses_before_a_device_is_needed_and_names_the_link(lib):
    """No context exists here: a non-null context pointer is never dereferenced before the checks are through (some
    host memory stands in).  A refused create leaves *out_tree NULL."""
    stand_in = np.zeros(64)
    ctx = capi._ptr(stand_in)
    handle = ctypes.c_void_p(1234)
    out = ctypes.byref(handle)

    def refused(needle, arrays=None, **kw):
        handle.value = 1234
        rc = (arrays or TreeArrays()).create(lib, kw.pop("ctx", ctx), kw.pop("out", out), **kw)
        message = lib.vgt_hip_last_error()
        assert rc == 1 and needle in message, (rc, message)
        assert handle.value is None
        return message

    refused(b"null", ctx=None)
    for name in ("parent", "joint_type", "joint_index", "axis", "origin"):
        refused(b"null", **{name: None})
    assert TreeArrays().create(lib, ctx, None) == 1 and b"null" in lib.vgt_hip_last_error()
    refused(b"at least one link", links=0)
    refused(b"at least one link", links=-3)
    refused(b"2^31", links=2 ** 31)
    refused(b"negative", joints=-1)
    # parents: -1 or below the link itself
    for link, bad in ((0, 0), (3, 3), (3, 5), (2, -2), (5, 2 ** 31 - 1)):
        a = TreeArrays()
        a.parent[link] = bad
        if link < 5:
            a.parent[5] = 7                                    # (the first offending link is the one named)
        message = refused(b"link %d: parent %d is not below %d" % (link, bad, link), a)
        assert link == 5 or b"link 5" not in message
    for bad in (3, -1, 99):
        a = TreeArrays()
        a.joint_type[4] = bad
        refused(b"link 4: joint type %d" % bad, a)
    for bad in (4, -1):
        a = TreeArrays()
        a.joint_index[3] = bad
        a.joint_index[2] = 77                                  # (a fixed link's index is ignored)
        refused(b"link 3: joint index %d is not in [0, 4)" % bad, a)
    # J == 0 with a link that is not fixed; whatever is wrong with the first bad link is what is reported
    refused(b"link 0: joint index 0 is not in [0, 0)", joints=0)
    a = TreeArrays()
    a.joint_type[1], a.parent[2] = 5, 2
    refused(b"link 1: joint type 5", a)


def test_forward_kinematics_argument_errors_and_empty_batch_without_device(lib):
    stand_in = np.zeros(64)
    ctx = tree = capi._ptr(stand_in)                           # (never dereferenced on these paths)
    q, poses, status = np.zeros((2, 4)), np.full((2, 6, 16), 7.0), np.full(2, 9, np.uint8)
    for fn in (lib.vgt_hip_forward_kinematics, lib.vgt_hip_forward_kinematics_dev):
        def call(ctx=ctx, tree=tree, q=capi._ptr(q), b=2, poses=capi._ptr(poses), status=capi._ptr(status)):
            return fn(ctx, tree, q, b, None, None, poses, status)

        assert call(ctx=None) == 1 and b"null" in lib.vgt_hip_last_error()
        assert call(tree=None) == 1 and b"null" in lib.vgt_hip_last_error()
        assert call(poses=None) == 1 and b"null" in lib.vgt_hip_last_error()
        for b in (-1, -(2 ** 40)):
            assert call(b=b) == 1 and b"negative" in lib.vgt_hip_last_error()
        for b in (2 ** 31, 2 ** 40):
            assert call(b=b) == 1 and b"2^31" in lib.vgt_hip_last_error()
        # nothing to do: success before the tree or the context is looked at
        assert call(b=0) == 0
        assert call(b=0, q=None, status=None) == 0
    assert (poses == 7.0).all() and (status == 9).all()


def test_joint_gradient_argument_errors_and_empty_batch_without_device(lib):
    stand_in = np.zeros(64)
    ctx = tree = capi._ptr(stand_in)
    p = capi._ptr(stand_in)
    out = np.full((2, 4), 7.0)
    for fn in (lib.vgt_hip_clearance_joint_gradient, lib.vgt_hip_clearance_joint_gradient_dev):
        def call(ctx=ctx, tree=tree, b=2, s=3, pairs=(p, p, None, None)):
            return fn(ctx, tree, p, b, p, p, s, *pairs, capi._ptr(out))

        assert call(ctx=None) == 1 and b"null" in lib.vgt_hip_last_error()
        assert call(tree=None) == 1 and b"null" in lib.vgt_hip_last_error()
        for pairs in ((None, None, None, None), (p, p, p, p), (p, None, None, None), (None, p, None, None),
                      (None, None, p, None), (p, p, p, None), (p, None, None, p)):
            assert call(pairs=pairs) == 1 and b"exactly one pair" in lib.vgt_hip_last_error()
        for kw in (dict(b=-1), dict(s=-1)):
            assert call(**kw) == 1 and b"negative" in lib.vgt_hip_last_error()
        for kw in (dict(b=2 ** 31), dict(s=2 ** 31)):
            assert call(**kw) == 1 and b"2^31" in lib.vgt_hip_last_error()
        assert call(b=0) == 0
        assert call(b=0, pairs=(None, None, p, p)) == 0
    assert (out == 7.0).all()


def test_chained_call_argument_errors_and_empty_batch_without_device(lib):
    stand_in = np.zeros(64)
    p = capi._ptr(stand_in)
    status = np.full(2, 9, np.uint8)

    def call(ctx=p, tree=p, b=2, st=capi._ptr(status)):
        return lib.vgt_hip_check_spheres_from_joints(ctx, p, 4, 4, 4, 0.1, None, None, p, p, 3, tree, p, b, None, None,
                                                     0.0, 0, st, *([None] * 9))

    assert call(ctx=None) == 1 and b"null" in lib.vgt_hip_last_error()
    assert call(tree=None) == 1 and b"null" in lib.vgt_hip_last_error()
    assert call(st=None) == 1 and b"null" in lib.vgt_hip_last_error()
    assert call(b=-1) == 1 and b"negative" in lib.vgt_hip_last_error()
    assert call(b=2 ** 31) == 1 and b"2^31" in lib.vgt_hip_last_error()
    assert call(b=0) == 0
    # a tree that is not this context's (the stand-in's zeroed bytes name no context at all)
    assert call() == 1 and b"another context" in lib.vgt_hip_last_error()
    assert lib.vgt_hip_forward_kinematics(p, p, p, 2, None, None, p, None) == 1
    assert b"another context" in lib.vgt_hip_last_error()
    assert (status == 9).all()


def test_handle_life_without_a_device(lib):
    """Destroying NULL is a no-op, the accessors answer 0 for NULL, and the Python object refuses before the library is
    asked: bad shapes, a closed tree."""
    lib.vgt_hip_kinematics_destroy(None)
    assert lib.vgt_hip_kinematics_num_links(None) == 0 and lib.vgt_hip_kinematics_num_joints(None) == 0

    class Stand(capi.Context):
        def __init__(self, lib, handle):
            self._lib, self.handle = lib, handle
            self.adopted = []

        def _adopt(self, child):
            self.adopted.append(child)

        def close(self):
            pass

    stand_in = np.zeros(64)
    ctx = Stand(lib, capi._ptr(stand_in))
    a = TreeArrays()
    with pytest.raises(ValueError, match="one parent, joint type"):
        ctx.kinematics(a.parent, a.joint_type[:5], a.joint_index, a.axis, a.origin)
    with pytest.raises(ValueError, match="one parent, joint type"):
        ctx.kinematics(a.parent, a.joint_type, a.joint_index, a.axis[:, :2], a.origin)
    with pytest.raises(ValueError, match=r"\[L, 16\] or \[L, 4, 4\]"):
        ctx.kinematics(a.parent, a.joint_type, a.joint_index, a.axis, np.zeros((6, 3, 4)))
    parent = a.parent.copy()
    parent[4] = 4
    with pytest.raises(ValueError, match="link 4: parent 4 is not below 4"):
        ctx.kinematics(parent, a.joint_type, a.joint_index, a.axis, a.origin.reshape(6, 4, 4))
    with pytest.raises(ValueError, match=r"link 4: joint index 3 is not in \[0, 3\)"):
        ctx.kinematics(a.parent, a.joint_type, a.joint_index, a.axis, a.origin, num_joints=3)
    assert not ctx.adopted
    # a tree that was closed (here: one that never came to be) is refused by the binding, and closing twice is harmless
    tree = capi.KinematicTree.__new__(capi.KinematicTree)
    tree.handle, tree.num_links, tree.num_joints, tree._lib = None, 6, 4, lib
    tree.close()
    tree.close()
    with pytest.raises(ValueError, match="closed"):
        ctx.forward_kinematics(tree, np.zeros((2, 4)))
    with pytest.raises(ValueError, match=r"\[B, 4\]"):
        ctx.forward_kinematics(tree, np.zeros((2, 3)))
    with pytest.raises(ValueError, match="closed"):
        ctx.clearance_joint_gradient(tree, np.zeros((2, 6, 16)), np.zeros((1, 4)), [0], min_sphere=[0, 0],
                                     min_gradient=np.zeros((2, 3)))
    with pytest.raises(ValueError, match="6 links"):
        ctx.clearance_joint_gradient(tree, np.zeros((2, 5, 16)), np.zeros((1, 4)), [0], min_sphere=[0, 0],
                                     min_gradient=np.zeros((2, 3)))
    # B == 0 through the binding, with a stand-in handle the library never looks at
    tree.handle = capi._ptr(stand_in)
    try:
        poses, status = ctx.forward_kinematics(tree, np.zeros((0, 4)))
        got = ctx.clearance_joint_gradient(tree, np.zeros((0, 6, 16)), np.zeros((1, 4)), [0], min_sphere=[],
                                           min_gradient=np.zeros((0, 3)))
    finally:
        tree.handle = None                                     # (nothing to destroy)
    assert poses.shape == (0, 6, 16) and status.shape == (0,) and status.dtype == np.uint8
    assert got.shape == (0, 4)
