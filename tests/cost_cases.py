"""Seeded inputs shared by tests/test_cost_ref.py and tests/test_gpu_cost.py: configurations of the trees of
tests/kinematics_cases.py in the scene of tests/body_cases.py, with the answers of tests/cost_ref.py computed once per case
and kept read-only.

Per case B = 67 configurations (for arm-21 also 1, T - 1, T, T + 1 and 257, T the kernel's tile for the arm's 8 links):
joint values uniform in +-1 with planted rows -- a NaN, an infinity, a value beyond 2^20, a row of zeros.  The margin is
0.25; arm-21 also runs with 2^-30, 1000 and a margin equal to a clearance that occurs (the `d == eps` edge), and once with
the radius of a sphere set to the bits of its own estimate in configuration 3, whose clearance is then exactly 0 there:
the order of `d < 0` and `d <= eps` decides the bits.  Sphere counts sit on both sides of the segment width 64 (64, 65, 70)
and of the kernel's sphere table (257 > 256).  Every second case passes joint limits.  The cases of FRAMED, appended,
run under a grid turned about a general axis and shifted.

coverage() states what the cases must hit, so that none passes by hitting nothing; tests/test_cost_ref.py asserts it."""
import collections
import functools
import os

import numpy as np

import body_cases
import cost_ref
import kinematics_cases
import motion_cases
import projection_cases

NUM_CONFIGURATIONS = 67
RESOLUTION = body_cases.RESOLUTION
MARGIN = 0.25
SEED = 5
EDGE = "edge"          # a margin equal to a clearance that occurs


def tile_samples():
    """T of the arm's 8 links (6 KiB / (96 B * 8) = 8 when the library is not built yet)."""
    from voxelized_geometry_tools_amd import capi
    if os.path.exists(capi.LIB_PATH):
        return capi.cost_tile_samples(8)
    return 8


def _cases():
    t = tile_samples()
    # (tree, S, odd field, B, margin, planted radius)
    out = [
        ("fixed1", 2, False, NUM_CONFIGURATIONS, MARGIN, False),
        ("arm", 1, False, NUM_CONFIGURATIONS, MARGIN, False),
        ("arm", 21, False, NUM_CONFIGURATIONS, MARGIN, False),
        ("arm", 64, True, NUM_CONFIGURATIONS, MARGIN, False),
        ("arm", 65, False, NUM_CONFIGURATIONS, MARGIN, False),
        ("arm", 70, False, NUM_CONFIGURATIONS, MARGIN, False),
        ("arm", 257, True, NUM_CONFIGURATIONS, MARGIN, False),
        ("body", 9, True, NUM_CONFIGURATIONS, MARGIN, False),
        ("braid-18", 6, True, NUM_CONFIGURATIONS, MARGIN, False),
        ("chain-41", 6, False, NUM_CONFIGURATIONS, MARGIN, False),
        ("chain-4", 5, False, NUM_CONFIGURATIONS, MARGIN, False),
        ("arm", 0, False, NUM_CONFIGURATIONS, MARGIN, False),
    ]
    out += [("arm", 21, False, b, MARGIN, False) for b in (1, t - 1, t, t + 1, 257)]
    out += [("arm", 21, False, NUM_CONFIGURATIONS, m, False) for m in (2.0 ** -30, 1000.0, EDGE)]
    out += [("arm", 21, True, NUM_CONFIGURATIONS, MARGIN, True)]
    return out


CASES = _cases()
# appended (the tests take cases by index, and index % 2 steers the limits): under the frame of
# tests/projection_cases.general_frame_pair() -- the grid turned about a general axis and shifted, grid_from_world and
# rotation passed, the tree on world_from_grid * world_from_base, so that it stays in the same part of the scene --
# arm-65-odd (several slices with the resting sums; its index is odd: with limits), arm-21 and the branching tree.  Every
# other case passes neither (None).
FRAMED = frozenset(range(len(CASES), len(CASES) + 3))
CASES += [
    ("arm", 65, True, NUM_CONFIGURATIONS, MARGIN, False),
    ("arm", 21, False, NUM_CONFIGURATIONS, MARGIN, False),
    ("body", 9, True, NUM_CONFIGURATIONS, MARGIN, False),
]
assert min(FRAMED) % 2 == 1

Case = collections.namedtuple(
    "Case", "name tree sdf xyzr link joint_values margin world_from_base joint_limits spheres want grid_from_world rotation")


def names():
    out = []
    for index, (tree, s, odd, b, margin, radius) in enumerate(CASES):
        name = "%s-%d%s" % (tree, s, "-odd" if odd else "")
        if index in FRAMED:
            name += "-frame"
        if b != NUM_CONFIGURATIONS:
            name += "-B%d" % b
        if margin != MARGIN:
            name += "-m-" + (margin if margin == EDGE else "%g" % margin)
        if radius:
            name += "-radius"
        out.append(name)
    return out


def joint_values(num, joints, seed=SEED):
    rng = np.random.default_rng(seed)
    q = rng.random((num, joints)) * 2.0 - 1.0
    if joints > 0 and num > 8:
        q[5, 0] = np.nan
        q[6, joints - 1] = np.inf
        q[7, 0] = np.nextafter(2.0 ** 20, np.inf)
        q[8] = 0.0
    return q


def model(tree, num_spheres):
    if num_spheres == 0:
        return np.zeros((0, 4)), np.zeros(0, np.int32)
    return kinematics_cases.sphere_model(tree, num_spheres, 31)


@functools.lru_cache(maxsize=None)
def case(index):
    from oracle import oracle as O
    tree_name, num_spheres, odd, num, margin, planted_radius = CASES[index]
    tree = kinematics_cases.tree(tree_name)
    sdf = body_cases.field(odd)
    xyzr, link = model(tree, num_spheres)
    q = joint_values(num, tree.num_joints)
    limits = kinematics_cases.limits(tree.num_joints) if index % 2 == 1 else None
    base = motion_cases.world_from_base()
    grid_from_world = rotation = None
    if index in FRAMED:
        grid_from_world, rotation, world_from_grid = projection_cases.general_frame_pair()
        base = projection_cases.base_under(world_from_grid, base)

    def spheres_at(eps):
        return cost_ref.spheres(O, sdf, RESOLUTION, xyzr, link, tree, q, eps, grid_from_world, rotation, base, limits)

    if planted_radius:
        # the estimate itself: the clearance of a sphere of radius 0; the first sphere whose estimate in configuration 3
        # is positive and finite takes it as its radius
        xyzr = xyzr.copy()
        probe = xyzr.copy()
        probe[:, 3] = 0.0
        estimate = cost_ref.spheres(O, sdf, RESOLUTION, probe, link, tree, q, MARGIN, None, None, base, limits).clearance[3]
        s = int(np.flatnonzero(np.isfinite(estimate) & (estimate > 0.0))[0])
        xyzr[s, 3] = estimate[s]
    if margin == EDGE:
        finite = np.sort(spheres_at(MARGIN).clearance.reshape(-1))
        finite = finite[np.isfinite(finite) & (finite > 0.0)]
        margin = float(finite[int(0.3 * (len(finite) - 1))])
    per_sphere = spheres_at(margin)
    want = cost_ref.reduce_spheres(tree, xyzr, link, per_sphere)
    if planted_radius:
        assert per_sphere.clearance[3, s] == 0.0 and not np.signbit(per_sphere.clearance[3, s])
    optional = [a for a in (limits, grid_from_world, rotation) if a is not None]
    for a in [xyzr, link, q, base] + list(per_sphere) + list(want) + optional:
        a.setflags(write=False)
    return Case(names()[index], tree, sdf, xyzr, link, q, margin, base, limits, per_sphere, want, grid_from_world, rotation)


def coverage(index):
    """(d < 0, 0 <= d <= eps, d > eps, without a value, active with a NaN gradient, d == eps) as sphere counts"""
    c = case(index)
    d = c.spheres.clearance
    with np.errstate(invalid="ignore"):
        value = ~np.isnan(d)
        active = value & (c.spheres.w != 0.0)
        return (int((d < 0.0).sum()), int(((d >= 0.0) & (d <= c.margin)).sum()), int((d > c.margin).sum()),
                int((~value).sum()), int((active & np.isnan(c.spheres.gradient).any(axis=2)).sum()),
                int((d == c.margin).sum()))
