"""Seeded inputs shared by tests/test_kinematics_ref.py and tests/test_gpu_kinematics.py: trees, joint values with
planted rows, limits and a base transform, with the answers of tests/kinematics_ref.py computed once per case.

Trees:
  fixed1      one fixed link
  arm         a serial arm, L = 8, J = 7: seven revolute links and a fixed tool (every parent is the link just before:
              the kernel's register path)
  body        L = 15: a prismatic torso lift on a fixed mount, a fixed shoulder bar, two arms of revolute links with a
              prismatic gripper each and fixed tool frames; the two gripper fingers of the left hand read one column
              (a mimic joint); axes of any length; links whose parent is not the link before (the kernel's LDS path)
  braid(n)    two interleaved chains, parent[i] = i - 2: no parent is the link before, and every link but the last two
              is such a parent.  With n = the kernel's LDS budget + 2 every parent's pose is in LDS (just inside the
              budget); with n = budget + 8 the six parents beyond it are read back from the output.  (The budget comes
              from the library: capi.kinematics_lds_links(), 10 when the library is not built -- the CPU tests do not
              depend on it.)
  chain(n)    a serial chain of the same two lengths

Joint values: uniform in +-pi, with planted rows (all columns): 0, -0.0, multiples of pi/2 and pi/4, +-2^20,
nextafter(2^20, inf), NaN, +-inf (in one column only, so that the other links are computed), values on and just beyond
the limits.
"""
import collections
import functools
import os

import numpy as np

import kinematics_ref as R

BATCHES = (1, 63, 64, 65, 257)
LIMIT = 2.5      # the limits are [-LIMIT, LIMIT] in every column but the last one, which is [-0.5, 0.25]

Case = collections.namedtuple("Case", "name tree joint_values world_from_base joint_limits poses status")


def lds_links():
    from voxelized_geometry_tools_amd import capi
    if os.path.exists(capi.LIB_PATH):
        return capi.kinematics_lds_links()
    return 10


def _origin(rng, scale=0.3):
    """[16] column-major: a random rotation and a translation of about `scale`"""
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    m = np.eye(4)
    m[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    m[:3, 3] = (rng.random(3) - 0.3) * scale
    out = m.T.reshape(16).copy()
    out[3::4] = [5.0, -5.0, np.nan, 2.0]           # (the row nobody reads)
    return out


def _unit(rng):
    a = rng.normal(size=3)
    return a / np.linalg.norm(a)


@functools.lru_cache(maxsize=None)
def tree(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    F, V, P = R.FIXED, R.REVOLUTE, R.PRISMATIC
    if name == "fixed1":
        return R.Tree([-1], [F], [0], [[0, 0, 1]], [_origin(rng)], 0)
    if name == "arm":
        parent = [-1, 0, 1, 2, 3, 4, 5, 6]
        kinds = [V] * 7 + [F]
        index = [0, 1, 2, 3, 4, 5, 6, 99]          # (a fixed link's index is ignored)
        axes = [[0, 0, 1], [0, 1, 0], [0, 0, 1], [0, -1, 0], [0, 0, 1], [0, 1, 0], [0, 0, 1], [0, 0, 0]]
        origins = [_origin(rng) for _ in range(8)]
        origins[0] = np.eye(4).reshape(16)         # (the first link at the base: an identity origin)
        return R.Tree(parent, kinds, index, axes, origins, 7)
    if name == "body":
        #          0 mount, 1 lift, 2 bar, | left: 3 4 5, 6 finger, 7 finger (mimic), 8 tool | right: 9 10 11, 12 finger, 13 tool, 14 camera on the bar
        parent = [-1, 0, 1, 2, 3, 4, 5, 5, 5, 2, 9, 10, 11, 11, 2]
        kinds = [F, P, F, V, V, V, P, P, F, V, V, V, P, F, V]
        index = [-7, 0, 0, 1, 2, 3, 4, 4, 0, 5, 6, 7, 8, 0, 9]
        axes = [_unit(rng) for _ in range(15)]
        axes[1] = np.array([0.0, 0.0, 1.0])
        axes[3] = axes[3] * 1.5                    # (used as they are: not unit)
        axes[7] = -axes[6] * 0.5
        axes[12] = axes[12] * 2.0
        return R.Tree(parent, kinds, index, axes, [_origin(rng) for _ in range(15)], 10)
    kind, _, count = name.partition("-")
    n = int(count)
    step = 2 if kind == "braid" else 1
    assert kind in ("braid", "chain")
    parent = [i - step if i >= step else -1 for i in range(n)]
    kinds = [(V, V, P, F)[i % 4] for i in range(n)]
    joints = 5
    index = [i % joints for i in range(n)]
    return R.Tree(parent, kinds, index, [_unit(rng) for _ in range(n)], [_origin(rng, 0.1) for _ in range(n)], joints)


def deep_names():
    k = lds_links()
    return ["braid-%d" % (k + 2), "braid-%d" % (k + 8), "chain-%d" % (k + 2), "chain-%d" % (k + 8)]


def joint_values(num, joints, seed):
    """[num, joints], the planted rows first as far as they fit, the rest uniform in +-pi"""
    rng = np.random.default_rng(seed)
    q = (rng.random((num, joints)) * 2.0 - 1.0) * np.pi
    if joints == 0:
        return q
    last = joints - 1
    planted = [np.zeros(joints), np.full(joints, -0.0)]
    planted += [np.full(joints, k * (np.pi / 2)) for k in (1, -1, 2, -3, 5)]
    planted += [np.arange(1, joints + 1) * (np.pi / 4) * s for s in (1.0, -1.0)]
    planted += [np.full(joints, LIMIT), np.full(joints, -LIMIT)]                        # on the limits
    planted += [np.full(joints, np.nextafter(LIMIT, np.inf)), np.full(joints, np.nextafter(-LIMIT, -np.inf))]
    for value in (2.0 ** 20, -2.0 ** 20, np.nextafter(2.0 ** 20, np.inf), np.nan, np.inf, -np.inf):
        row = q[len(planted) % num].copy()
        row[0] = value
        planted.append(row)
        row = q[(len(planted) + 1) % num].copy()
        row[last] = value
        planted.append(row)
    on_last = np.zeros(joints)
    on_last[last] = 0.25
    beyond_last = np.zeros(joints)
    beyond_last[last] = np.nextafter(0.25, np.inf)
    planted += [on_last, beyond_last, np.full(joints, 2.0 ** 20)]
    if num >= len(planted):
        q[:len(planted)] = planted
    else:                                          # small batches: what fits, the harshest rows first
        for i in range(num):
            q[i] = planted[(len(planted) - 1 - 3 * i) % len(planted)]
    return q


def limits(joints):
    out = np.tile([-LIMIT, LIMIT], (joints, 1)).astype(np.float64)
    if joints:
        out[-1] = [-0.5, 0.25]
    return out


def base_transform():
    out = _origin(np.random.default_rng(5), 2.0)
    out[3::4] = [9.0, 9.0, 9.0, 9.0]
    return out


def tree_names():
    return ["fixed1", "arm", "body"] + deep_names()


def all_cases():
    """(tree name, B, with base, with limits): every tree at every batch size, the two options alternating; the deep
    trees at B = 65 and 257 only."""
    out = []
    for t, name in enumerate(tree_names()):
        for k, num in enumerate(BATCHES):
            if t >= 3 and num not in (65, 257):
                continue
            out.append((name, num, (t + k) % 2 == 0, (t + k) % 3 != 1))
    return out


def case_names():
    return ["%s-B%d%s%s" % (n, b, "-base" if base else "", "-limits" if lim else "") for n, b, base, lim in all_cases()]


@functools.lru_cache(maxsize=None)
def case(index):
    name, num, with_base, with_limits = all_cases()[index]
    t = tree(name)
    q = joint_values(num, t.num_joints, 300 + index)
    base = base_transform() if with_base else None
    lim = limits(t.num_joints) if with_limits else None
    poses, status = R.forward_kinematics(t, q, base, lim)
    for a in (q, poses, status) + ((base,) if with_base else ()) + ((lim,) if with_limits else ()):
        a.setflags(write=False)
    return Case(case_names()[index], t, q, base, lim, poses, status)


def sphere_model(t, num_spheres, seed):
    """(xyzr [S, 4], link [S] int32): links in no order, one sphere at its link's origin"""
    rng = np.random.default_rng(seed)
    xyzr = np.empty((num_spheres, 4))
    xyzr[:, :3] = (rng.random((num_spheres, 3)) - 0.5) * 0.4
    xyzr[:, 3] = rng.random(num_spheres) * 0.1
    xyzr[0, :3] = 0.0
    link = rng.integers(0, t.num_links, num_spheres).astype(np.int32)
    link[-1] = t.num_links - 1
    return xyzr, link


GradientCase = collections.namedtuple(
    "GradientCase", "name tree poses xyzr link min_sphere min_gradient weight gradient want_worst want_summed")

# (index into all_cases() by name, spheres)
GRADIENT_CASES = [("fixed1", 65, 3), ("arm", 1, 5), ("arm", 65, 12), ("arm", 257, 7), ("body", 64, 9), ("body", 257, 12)]


def gradient_case_names():
    return ["%s-B%d-S%d" % c for c in GRADIENT_CASES] + ["deep-B65-S6"]


@functools.lru_cache(maxsize=None)
def gradient_case(index):
    """What the check would return for the shared poses (NaN links included), made up: a worst sphere per
    configuration (with -1, S and a sphere on a link outside [0, L) planted) and its gradient; weights with zeros (their
    gradients NaN), a NaN weight, a -0.0 weight, and gradients with a NaN row."""
    if index < len(GRADIENT_CASES):
        name, num, count = GRADIENT_CASES[index]
    else:
        name, num, count = deep_names()[1], 65, 6
    found = [i for i, c in enumerate(all_cases()) if c[0] == name and c[1] == num]
    fk = case(found[0])
    t = fk.tree
    rng = np.random.default_rng(900 + index)
    xyzr, link = sphere_model(t, count, 700 + index)
    if count > 4:
        link[2] = t.num_links                      # a link outside [0, L)
        link[3] = -1
    min_sphere = rng.integers(0, count, num).astype(np.int32)
    min_gradient = rng.normal(size=(num, 3))
    weight = rng.random((num, count))
    weight[rng.random((num, count)) < 0.4] = 0.0
    gradient = rng.normal(size=(num, count, 3))
    gradient[weight == 0.0] = np.nan
    if num > 8:
        min_sphere[1], min_sphere[2], min_sphere[3] = -1, count, 2 if count > 4 else 0
        min_gradient[4] = np.nan
        weight[5, 0], weight[6, 1] = np.nan, -0.0
        gradient[7, count - 1] = [np.nan, 1.0, np.inf]
        weight[7, count - 1] = 0.5
    want_worst = R.clearance_joint_gradient(t, fk.poses, xyzr, link, min_sphere=min_sphere, min_gradient=min_gradient)
    want_summed = R.clearance_joint_gradient(t, fk.poses, xyzr, link, sphere_weight=weight, sphere_gradient=gradient)
    for a in (xyzr, link, min_sphere, min_gradient, weight, gradient, want_worst, want_summed):
        a.setflags(write=False)
    return GradientCase(gradient_case_names()[index], t, fk.poses, xyzr, link, min_sphere, min_gradient, weight,
                        gradient, want_worst, want_summed)
