"""Seeded inputs shared by tests/test_align_ref.py and tests/test_gpu_align.py, with the answers of tests/align_ref.py
computed once per case.

The scene is a 32 x 28 x 36 grid at resolution 0.05: two boxes (one of them a slab with a large flat face) and two
spheres; its field is the CPU oracle's SDF (which the device's extraction equals bit for bit, tests/test_gpu_sdf.py).  A
cloud is made of centres of surface cells (filled cells with a free face neighbour), moved into the sensor's frame by
the inverse of a known pose: `truth()` is then the world_from_points that aligns it.  `wall()` is the field of one
axis-aligned slab alone, in which the interpolant's gradient has two components that are exactly zero.

The GPU cases (SHAPES: N points, B poses, K steps) use clouds of any size drawn from those centres with a jitter of
+-0.4 cell, and put into every cloud of more than 16 points a NaN point, an infinite one, points outside the grid and
points in free space whose residual exceeds max_residual; every second case runs under an origin transform (rotated and
shifted: tests/projection_cases.frame_pair), every third one without a pivot.  In every batch of more than two poses: pose 1
sends the cloud out of the grid (TOO_FEW); the last pose has a zero rotation block and puts every point at one place
in front of the slab's face (DEGENERATE, when K > 0); the others start from the truth moved by 0 to 5 cells and 0 to 10
degrees, so that with the tolerances used some converge after two steps and some run to the limit.
"""
import collections
import functools

import numpy as np

import align_ref
import projection_cases

SHAPE = (32, 28, 36)
RESOLUTION = 0.05

# (N, B, K): every N, B and K of the list below at least once; 4097 and 8197 points are two and three blocks of 4096.
# The last case has 257 * 3 = 771 (pose, block) items: more than 768, from where on the evaluation runs in its form with
# four waves per workgroup (csrc/align_kernels.hip, kAlignWideItems); every other case runs the form with sixteen.
SHAPES = [
    (1, 1, 0), (63, 3, 1), (64, 1, 8), (65, 3, 0), (257, 67, 1), (257, 3, 8), (4097, 1, 1), (4097, 3, 8), (8197, 1, 0),
    (8197, 3, 1), (8197, 67, 8), (64, 67, 0), (8197, 257, 1),
]

Case = collections.namedtuple(
    "Case", "name sdf resolution points poses options grid_from_world rotation want")


def _occupancy(slab_only):
    occ = np.zeros(SHAPE, dtype=np.float32)
    occ[3:7, 4:24, 6:30] = 1.0                                                     # the slab
    if slab_only:
        return occ
    occ[20:26, 3:8, 5:12] = 1.0
    x, y, z = np.meshgrid(*[np.arange(n) + 0.5 for n in SHAPE], indexing="ij")
    occ[(x - 20.0) ** 2 + (y - 18.0) ** 2 + (z - 24.0) ** 2 <= 5.0 ** 2] = 1.0
    occ[(x - 23.0) ** 2 + (y - 19.5) ** 2 + (z - 9.0) ** 2 <= 4.0 ** 2] = 1.0
    return occ


@functools.lru_cache(maxsize=None)
def _field(slab_only):
    from oracle import oracle as O
    sdf, _, _ = O.sdf_from_occupancy(_occupancy(slab_only), RESOLUTION)
    sdf = sdf.copy()
    sdf.setflags(write=False)
    return sdf


def scene():
    return _field(False)


def wall():
    return _field(True)


@functools.lru_cache(maxsize=None)
def surface_centres(slab_only=False):
    """Centres [M, 3] float64, in the grid's frame, of the filled cells with a free face neighbour."""
    filled = _occupancy(slab_only) > 0.5
    free = np.pad(~filled, 1, constant_values=False)
    near = (free[2:, 1:-1, 1:-1] | free[:-2, 1:-1, 1:-1] | free[1:-1, 2:, 1:-1] | free[1:-1, :-2, 1:-1] |
            free[1:-1, 1:-1, 2:] | free[1:-1, 1:-1, :-2])
    centres = (np.argwhere(filled & near).astype(np.float64) + 0.5) * RESOLUTION
    centres.setflags(write=False)
    return centres


def centre():
    """The grid's centre in its own frame."""
    return np.array(SHAPE, dtype=np.float64) * RESOLUTION * 0.5


def rotation_about(axis, degrees):
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    a = np.radians(degrees)
    K = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def matrix(R, t):
    m = np.eye(4)
    m[:3, :3] = R
    m[:3, 3] = t
    return m


def column_major(m):
    return np.ascontiguousarray(m.T).reshape(16).copy()


def truth():
    """world_from_points (4 x 4, the grid's frame as the world) of every cloud made here."""
    return matrix(rotation_about([0.3, -0.5, 0.8], 25.0), [0.31, 0.52, -0.17])


def moved(pose, cells, degrees, seed):
    """`pose` turned by `degrees` about a seeded axis through the grid's centre and shifted by `cells` cells."""
    rng = np.random.default_rng(seed)
    R = rotation_about(rng.normal(size=3), degrees)
    direction = rng.normal(size=3)
    shift = direction / np.linalg.norm(direction) * cells * RESOLUTION
    c = centre()
    return matrix(R, c - R @ c + shift) @ pose


def to_cloud(world_points):
    """float32 points in the sensor's frame"""
    inverse = np.linalg.inv(truth())
    return (world_points @ inverse[:3, :3].T + inverse[:3, 3]).astype(np.float32)


def surface_cloud(slab_only=False):
    return to_cloud(surface_centres(slab_only))


def cloud(num_points, seed):
    """num_points float32 points: jittered surface centres, and (from 17 points on) the odd ones of the module's text."""
    rng = np.random.default_rng(seed)
    centres = surface_centres()
    world = centres[rng.integers(0, len(centres), num_points)] + (rng.random((num_points, 3)) - 0.5) * 0.8 * RESOLUTION
    if num_points > 16:
        world[3] = [-0.4, 0.3, 0.5]                                                # outside the grid
        world[num_points - 2] = [0.8, 0.7, 2.5]
        world[5] = [0.6, 0.65, 0.9]                                                # free space, cells away from anything
        world[num_points // 2] = [0.65, 0.2, 1.3]
    points = to_cloud(world)
    if num_points > 16:
        points[7] = [np.nan, 0.1, 0.2]
        points[num_points - 1] = [0.3, np.inf, 0.1]
        points[num_points // 3] = [0.1, 0.2, -np.inf]
    return points


def start_poses(num_poses, seed, world_from_grid):
    """[B, 16] column-major, in the world frame"""
    out = np.empty((num_poses, 16))
    for b in range(num_poses):
        scale = (b % 5) / 4.0                                                      # 0, 1/4 ... 1
        pose = moved(truth(), 5.0 * scale, 10.0 * scale, seed * 1000 + b)
        if num_poses > 2 and b == 1:
            pose = matrix(np.eye(3), [3.0, -2.0, 1.0]) @ pose
        if num_poses > 2 and b == num_poses - 1:
            pose = matrix(np.zeros((3, 3)), [0.37, 0.7, 0.9])                      # just in front of the slab's face
        out[b] = column_major(world_from_grid @ pose)
    out[:, 3::4] = [7.0, -7.0, np.nan, 3.0]                                        # (the row nobody reads)
    return out


@functools.lru_cache(maxsize=None)
def case(index):
    num_points, num_poses, steps = SHAPES[index]
    sdf = scene()
    points = cloud(num_points, 300 + index)
    grid_from_world = rotation = None
    world_from_grid = np.eye(4)
    if index % 2 == 1:
        grid_from_world, rotation, world_from_grid = projection_cases.frame_pair()
    pivot = None
    if index % 3 != 2:
        pivot = world_from_grid[:3, :3] @ centre() + world_from_grid[:3, 3]
    poses = start_poses(num_poses, index, world_from_grid)
    options = dict(max_iterations=steps, min_points=6, damping=1e-3, max_residual=1.5 * RESOLUTION,
                   target_distance=-0.5 * RESOLUTION, translation_tolerance=2e-3 * RESOLUTION,
                   rotation_tolerance=1e-4, pivot=pivot)
    want = align_ref.align(sdf, RESOLUTION, points, poses, grid_from_world=grid_from_world, rotation=rotation, **options)
    for a in (points, poses, *want):
        a.setflags(write=False)
    return Case("N%d-B%d-K%d" % SHAPES[index], sdf, RESOLUTION, points, poses, options, grid_from_world, rotation, want)


def names():
    return ["N%d-B%d-K%d" % s for s in SHAPES]
