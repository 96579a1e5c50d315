"""Seeded inputs shared by tests/test_ik_ref.py and tests/test_gpu_ik.py: (tree, tip) pairs, targets that are the forward
kinematics of rows drawn inside the limits, seeds around the truth, planted rows, and the answers of tests/ik_ref.py
computed once per case.

Trees (tests/kinematics_cases.py): `arm` with tip 7 (all seven columns on the chain), `body` with tip 13 (the right arm:
lift + three revolute links of unit axes; six columns off the chain, the left hand's mimic pair among them) and `body`
with tip 8 (link 3's axis has length 1.5: its columns are no derivatives -- bit-equality only).  serial(n): a fresh
serial chain of n moving links, one column each, with two fixed links in between; n = the kernel's constant
(capi.ik_max_chain_joints(), 16 when the library is not built) is the longest chain the call takes, n + 1 is refused.

Planted rows (batches of 16 and more):
  0   the seed is the solution
  1   the target is the seed's pose turned half a turn about the tip's x axis
  2   NaN in a column a revolute chain link reads          3   nextafter(2^20, inf) there
  4   NaN in a column no chain link reads (trees that have one)     5   nextafter(2^20, inf) there
"""
import collections
import functools
import os

import numpy as np

import ik_ref
import kinematics_cases as KC
import kinematics_ref as R

BATCHES = (1, 63, 64, 65, 257)

Case = collections.namedtuple(
    "Case", "name tree tip targets seeds_per_target seeds truth world_from_base joint_limits options want")

DEFAULTS = dict(task_weights=None, max_iterations=50, damping=0.01, max_step=0.5, position_tolerance=1e-6,
                rotation_tolerance=1e-6)


def max_chain_joints():
    from voxelized_geometry_tools_amd import capi
    if os.path.exists(capi.LIB_PATH):
        return capi.ik_max_chain_joints()
    return 16


@functools.lru_cache(maxsize=None)
def serial(moving):
    """A serial chain of `moving` links that are not fixed (revolute, revolute, prismatic in turn; unit axes), one column
    each, and two fixed links: after the first link and at the tip."""
    rng = np.random.default_rng(1000 + moving)
    kinds, index = [], []
    for k in range(moving):
        kinds.append((R.REVOLUTE, R.REVOLUTE, R.PRISMATIC)[k % 3])
        index.append(k)
        if k == 0:
            kinds.append(R.FIXED)
            index.append(0)
    kinds.append(R.FIXED)
    index.append(0)
    n = len(kinds)
    parent = [i - 1 for i in range(n)]
    return R.Tree(parent, kinds, index, [KC._unit(rng) for _ in range(n)], [KC._origin(rng, 0.1) for _ in range(n)],
                  moving)


def tree(name):
    if name.startswith("serial-"):
        return serial(int(name.partition("-")[2]))
    return KC.tree(name)


def _on_and_off_chain(t, tip):
    """(a column a revolute chain link reads, a column no chain link reads or None)"""
    moving = ik_ref.moving_links(t, tip)
    on = [int(t.joint_index[i]) for i in moving if int(t.joint_type[i]) == R.REVOLUTE][0]
    read = {int(t.joint_index[i]) for i in moving}
    off = [j for j in range(t.num_joints) if j not in read]
    return on, (off[0] if off else None)


# name: (tree, tip, T, R, spread of the seeds, with base, limits (None, "wide" = kinematics_cases.limits, or a half
# width), options that differ from DEFAULTS)
CASES = collections.OrderedDict([
    ("arm-near-B1", ("arm", 7, 1, 1, 0.1, False, None, {})),
    ("arm-near-B63-R3", ("arm", 7, 21, 3, 0.1, False, "wide", {})),
    ("arm-near-B64-base", ("arm", 7, 64, 1, 0.1, True, None, {})),
    ("arm-0.3-B65-limits", ("arm", 7, 65, 1, 0.3, False, "wide", {})),
    ("arm-1.0-B257", ("arm", 7, 257, 1, 1.0, True, "wide", {})),
    ("arm-K0-B63", ("arm", 7, 63, 1, 0.1, False, None, dict(max_iterations=0))),
    ("arm-small-step-B64", ("arm", 7, 64, 1, 0.3, False, None, dict(max_step=0.01, max_iterations=12))),
    ("arm-tight-limits-B65", ("arm", 7, 65, 1, 1.0, False, 0.6, dict(max_step=float("inf")))),
    ("body13-near-B257", ("body", 13, 257, 1, 0.1, True, "wide", {})),
    ("body13-position-only-B65", ("body", 13, 65, 1, 0.3, False, None, dict(task_weights=(1, 1, 1, 0, 0, 0)))),
    ("body13-undamped-B64", ("body", 13, 64, 1, 0.1, False, None, dict(damping=0.0))),
    ("body13-weights-R3-B63", ("body", 13, 21, 3, 0.3, False, "wide", dict(task_weights=(1, 2, 0.5, 0.25, 0, 1)))),
    ("body8-0.3-B65", ("body", 8, 65, 1, 0.3, True, None, dict(max_iterations=20))),
    ("serial-longest-B65", ("serial", -1, 65, 1, 0.1, False, None, dict(max_iterations=10))),
])


def case_names():
    return list(CASES)


def _limits(t, kind):
    if kind is None:
        return None
    if kind == "wide":
        return KC.limits(t.num_joints)
    return np.tile([-kind, kind], (t.num_joints, 1)).astype(np.float64)


def problem(name, spec=None):
    """Everything of a case but the answer; spec: a row like those of CASES for a name that is not there."""
    tree_name, tip, num_targets, per_target, spread, with_base, limit_kind, changed = spec or CASES[name]
    if tree_name == "serial":
        tree_name = "serial-%d" % max_chain_joints()
    t = tree(tree_name)
    if tip < 0:
        tip = t.num_links - 1
    rng = np.random.default_rng(sum(map(ord, name)))
    limits = _limits(t, limit_kind)
    box = limits if limits is not None else KC.limits(t.num_joints)
    base = KC.base_transform() if with_base else None
    truth = box[:, 0] + rng.random((num_targets, t.num_joints)) * (box[:, 1] - box[:, 0])
    poses, _ = R.forward_kinematics(t, truth, base, None)
    targets = np.ascontiguousarray(poses[:, tip])
    num = num_targets * per_target
    truth = np.repeat(truth, per_target, axis=0)
    seeds = truth + (rng.random((num, t.num_joints)) * 2.0 - 1.0) * spread
    if limits is not None:
        seeds = np.minimum(np.maximum(seeds, limits[:, 0]), limits[:, 1])
    if num >= 16 and per_target == 1:
        on, off = _on_and_off_chain(t, tip)
        seeds[0] = truth[0]
        turned, _ = R.forward_kinematics(t, seeds[1:2], base, None)
        targets[1] = turned[0, tip]
        targets[1, 4:7] = -targets[1, 4:7]
        targets[1, 8:11] = -targets[1, 8:11]
        seeds[2, on] = np.nan
        seeds[3, on] = np.nextafter(2.0 ** 20, np.inf)
        if off is not None:
            seeds[4, off] = np.nan
            seeds[5, off] = np.nextafter(2.0 ** 20, np.inf)
    options = dict(DEFAULTS)
    options.update(changed)
    return t, tip, targets, per_target, seeds, truth, base, limits, options


@functools.lru_cache(maxsize=None)
def case(name):
    t, tip, targets, per_target, seeds, truth, base, limits, options = problem(name)
    want = ik_ref.solve_ik(t, tip, targets, seeds, per_target, base, limits, **options)
    for a in (targets, seeds, truth) + tuple(want) + tuple(x for x in (base, limits) if x is not None):
        a.setflags(write=False)
    return Case(name, t, tip, targets, per_target, seeds, truth, base, limits, options, want)
