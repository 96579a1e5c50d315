"""Seeded inputs shared by tests/test_motion_ref.py and tests/test_gpu_motions.py: motions of the trees of
tests/kinematics_cases.py through the scene of tests/body_cases.py, with the answers of tests/motion_ref.py computed once
per case and kept read-only.

Per case E = 67 motions: joint_from uniform in +-1, joint_to = joint_from + uniform in +-1.5; step counts
STEPS[e % 17], on both sides of the tile sizes 8, 16, 32 and 64 (the trees make the kernel choose 64, 32, 16, 8, 4 and
2), 2615 samples in all; planted rows (J > 0): a NaN and a value beyond 2^20 in joint_from, an infinity in joint_to, a
motion that goes nowhere.
minimum_clearance is a clearance that occurs (the `<=` edge, as in tests/body_cases.py): the stated quantile of the sorted
finite per-sample min_clearance at threshold 0.  Every second case passes joint limits; every third replaces num_steps by
uniform_steps = 33.

The cases of FRAMED run under tests/projection_cases.general_frame_pair(): the grid turned about a general axis and
shifted, grid_from_world and rotation passed, and the tree on world_from_grid * world_from_base, so that it moves through
the same part of the scene as without the frame.  Every other case passes neither (None).  The two models of 257 spheres
are larger than the kernel's LDS table (tests/test_gpu_motions.py asserts with the launcher's own geometry that they are
read through the cache)."""
import collections
import functools

import numpy as np

import body_cases
import kinematics_cases
import motion_ref
import projection_cases

NUM_MOTIONS = 67
STEPS = (0, 1, 2, 3, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130, 200)
UNIFORM_STEPS = 33
RESOLUTION = body_cases.RESOLUTION

# (tree, S, odd field, quantile, outside-is-collision)
CASES = [
    ("arm", 21, False, 0.01, False),
    ("arm", 21, True, 0.02, True),
    ("body", 9, False, 0.01, False),
    ("body", 9, True, 0.02, True),
    ("arm", 70, False, 0.01, False),
    ("arm", 3, True, 0.02, False),
    ("fixed1", 2, False, 0.5, False),
    ("chain-18", 6, False, 0.01, False),
    ("braid-18", 6, True, 0.02, True),
    ("chain-41", 6, False, 0.01, False),
    ("chain-4", 5, False, 0.01, False),          # (a tile of 32 samples under the kernel's 12 KiB of poses)
]
# appended (the tests take cases by index, and index % 2 and index % 3 steer limits and uniform steps): under the frame
# arm-21 with limits, the branching tree on the odd field with outside-is-collision, arm-257-odd; arm-257 without one
FRAMED = frozenset((len(CASES), len(CASES) + 1, len(CASES) + 3))
CASES += [
    ("arm", 21, False, 0.01, False),
    ("body", 9, True, 0.02, True),
    ("arm", 257, False, 0.01, False),
    ("arm", 257, True, 0.02, False),
]

Case = collections.namedtuple(
    "Case", "name tree sdf xyzr link joint_from joint_to num_steps minimum_clearance outside_is_collision world_from_base "
            "joint_limits samples first want want_stopped grid_from_world rotation")


def names():
    return ["%s-%d%s%s" % (tree, s, "-odd" if odd else "", "-frame" if index in FRAMED else "")
            for index, (tree, s, odd, _, _) in enumerate(CASES)]


def world_from_base():
    base = np.eye(4)
    base[:3, 3] = [1.5, 1.25, 1.0]
    return base.T.reshape(16).copy()


def endpoints(num_joints):
    rng = np.random.default_rng(77)
    joint_from = (rng.random((NUM_MOTIONS, num_joints)) * 2.0 - 1.0) * 1.0
    joint_to = joint_from + (rng.random((NUM_MOTIONS, num_joints)) * 2.0 - 1.0) * 1.5
    if num_joints > 0:
        joint_from[5, 0] = np.nan
        joint_to[6, num_joints - 1] = np.inf
        joint_from[7, 0] = np.nextafter(2.0 ** 20, np.inf)
        joint_to[8] = joint_from[8]
    return joint_from, joint_to


@functools.lru_cache(maxsize=None)
def case(index):
    from oracle import oracle as O
    tree_name, num_spheres, odd, quantile, outside = CASES[index]
    tree = kinematics_cases.tree(tree_name)
    sdf = body_cases.field(odd)
    xyzr, link = kinematics_cases.sphere_model(tree, num_spheres, 31)
    joint_from, joint_to = endpoints(tree.num_joints)
    if index % 3 == 2:
        num_steps = UNIFORM_STEPS
    else:
        num_steps = np.array([STEPS[e % len(STEPS)] for e in range(NUM_MOTIONS)], dtype=np.int32)
    limits = kinematics_cases.limits(tree.num_joints) if index % 2 == 1 else None
    base = world_from_base()
    grid_from_world = rotation = None
    if index in FRAMED:
        grid_from_world, rotation, world_from_grid = projection_cases.general_frame_pair()
        base = projection_cases.base_under(world_from_grid, base)
    q, first = motion_ref.interpolate(joint_from, joint_to, num_steps)

    def samples_at(threshold):
        return motion_ref.check_samples(O, sdf, RESOLUTION, xyzr, link, tree, q, threshold, outside, grid_from_world,
                                        rotation, base, limits)

    finite = np.sort(samples_at(0.0).min_clearance)
    finite = finite[np.isfinite(finite)]
    minimum_clearance = float(finite[int(quantile * (len(finite) - 1))])
    samples = samples_at(minimum_clearance)
    want = motion_ref.reduce_motions(samples, first, False)
    want_stopped = motion_ref.reduce_motions(samples, first, True)
    arrays = [xyzr, link, joint_from, joint_to, base, first] + list(samples) + list(want) + list(want_stopped)
    arrays += [a for a in (num_steps, limits, grid_from_world, rotation) if isinstance(a, np.ndarray)]
    for a in arrays:
        a.setflags(write=False)
    return Case(names()[index], tree, sdf, xyzr, link, joint_from, joint_to, num_steps, minimum_clearance, outside, base,
                limits, samples, first, want, want_stopped, grid_from_world, rotation)
