"""Scenes and segments shared by tests/test_segment_ref.py and tests/test_gpu_segments.py: the reference test's 1000
origin/point pairs on a 40^3 scene, known answers written out by hand, and the smallest grids at which the walk of
vgt_hip_cast_segments can go wrong."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE_COUNTS = (40, 40, 40)
FIXTURE_RESOLUTION = 0.125


def fixture_segments():
    """tests/golden/raycast_rays.npy, the pairs of the reference's test/voxel_raycasting_test.cpp: [1000, 6]."""
    return np.load(os.path.join(GOLDEN, "raycast_rays.npy"))


def fixture_occupancy():
    """40^3: the box [16, 24)^3 filled, the floor z = 0 filled, the plane x = 30 unknown (0.5)."""
    occ = np.zeros(FIXTURE_COUNTS, dtype=np.float32)
    occ[16:24, 16:24, 16:24] = 1.0
    occ[:, :, 0] = 1.0
    occ[30, :, :] = 0.5
    return occ


def linear(counts, cell):
    return (cell[0] * counts[1] + cell[1]) * counts[2] + cell[2]


# ---- known answers written out by hand ----
# (name, counts, filled cells, segment, status, hit cell or None, cells examined, hit fraction or None, cells or None)
NAN, INF = math.nan, math.inf
DIAGONAL = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 2, 2), (3, 2, 2), (3, 3, 2), (3, 3, 3)]
HAND_CASES = [
    ("column up", (1, 1, 4), [(0, 0, 2)], (0.5, 0.5, 0.25, 0.5, 0.5, 3.75), 1, (0, 0, 2), 3, 0.5, None),
    ("column down", (1, 1, 4), [(0, 0, 2)], (0.5, 0.5, 3.75, 0.5, 0.5, 0.25), 1, (0, 0, 2), 2, 0.75 / 3.5, None),
    ("diagonal, ties X Y Z", (4, 4, 4), [], (0.5, 0.5, 0.5, 3.5, 3.5, 3.5), 0, None, 10, None, DIAGONAL),
    ("through the grid", (4, 4, 4), [], (-1.5, 0.5, 0.5, 5.5, 0.5, 0.5), 0, None, 4, None,
     [(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)]),
    ("ends before the grid", (4, 4, 4), [], (-3.0, 0.5, 0.5, -1.0, 0.5, 0.5), 2, None, 0, None, []),
    ("touches the upper face", (4, 4, 4), [], (5.0, 0.5, 0.5, 4.0, 0.5, 0.5), 2, None, 0, None, []),
    ("leaves through the upper face", (4, 4, 4), [], (3.5, 0.5, 0.5, 4.0, 0.5, 0.5), 0, None, 1, None, [(3, 0, 0)]),
    ("zero length inside", (4, 4, 4), [], (1.5, 2.5, 3.5, 1.5, 2.5, 3.5), 0, None, 1, None, [(1, 2, 3)]),
    ("zero length outside", (4, 4, 4), [], (-1.0, 0.5, 0.5, -1.0, 0.5, 0.5), 2, None, 0, None, []),
    ("NaN coordinate", (4, 4, 4), [], (0.5, NAN, 0.5, 3.5, 0.5, 0.5), 3, None, 0, None, None),
    ("infinite coordinate", (4, 4, 4), [], (0.5, 0.5, 0.5, INF, 0.5, 0.5), 3, None, 0, None, None),
    ("infinite origin", (4, 4, 4), [], (-INF, 0.5, 0.5, 0.5, 0.5, 0.5), 3, None, 0, None, None),
]
HAND_RESOLUTION = 1.0


def hand_field(counts, filled):
    occ = np.zeros(counts, dtype=np.float32)
    for cell in filled:
        occ[cell] = 1.0
    return occ


# ---- degenerate grids ----
DEGENERATE_COUNTS = [(1, 1, 1), (1, 1, 7), (3, 2, 5), (1, 40, 1)]


def degenerate_case(counts, seed=5):
    """(occupancy with a third of the cells filled and a few unknown, resolution, [96, 6] segments with ends in and
    around the grid's box, some on cell faces and corners, some of length zero)."""
    rng = np.random.default_rng(seed + 31 * sum(counts))
    res = 0.25
    occ = np.zeros(counts, dtype=np.float32)
    pick = rng.random(counts)
    occ[pick < 0.33] = 1.0
    occ[pick > 0.9] = 0.5
    size = np.array(counts, dtype=np.float64) * res
    ends = rng.uniform(-0.5, 1.5, size=(96, 2, 3)) * size
    ends[:24] = np.round(ends[:24] / res) * res         # on faces, edges and corners of cells
    ends[24:32, 1] = ends[24:32, 0]                     # length zero
    ends[32:48, 1, 0] = ends[32:48, 0, 0]               # flat along x
    ends[48:56, 1, :2] = ends[48:56, 0, :2]             # along z only
    return occ, res, ends.reshape(96, 6)


def rotated_frame():
    """grid_from_world (16 doubles column-major) of a grid rotated about a skew axis and shifted, and world_from_grid
    as a 4 x 4 matrix."""
    axis = np.array([0.3, -0.5, 0.8])
    axis /= np.linalg.norm(axis)
    angle = 0.7
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R = np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)
    world_from_grid = np.eye(4)
    world_from_grid[:3, :3] = R
    world_from_grid[:3, 3] = (1.25, -0.5, 2.0)
    grid_from_world = np.linalg.inv(world_from_grid)
    return np.ascontiguousarray(grid_from_world.T).reshape(16), world_from_grid


def to_world(segments, world_from_grid):
    seg = np.asarray(segments, dtype=np.float64).reshape(-1, 2, 3)
    return (seg @ world_from_grid[:3, :3].T + world_from_grid[:3, 3]).reshape(-1, 6)
