"""Scenes and query clouds shared by tests/test_projection_ref.py and tests/test_gpu_projection.py: the smallest shapes at
which each branch of the projection out of collision (tests/projection_ref.py) can go wrong.  Fields come from the CPU
oracle's SDF, which the device's extraction equals bit for bit (tests/test_gpu_sdf.py)."""
import functools

import numpy as np

from voxelized_geometry_tools_amd import synthetic


def query_cloud(shape, res, n, seed):
    """n points uniform in [-0.1, 1.1) x the grid's extent, every 17th on a cell boundary, one NaN and one infinite."""
    rng = np.random.default_rng(seed)
    extent = np.array(shape, dtype=np.float64) * res
    q = (rng.random((n, 3)) * 1.2 - 0.1) * extent
    q[::17] = np.floor(q[::17] / res) * res
    q[5] = [np.nan, 0.1, 0.1]
    q[6] = [np.inf, 0.1, 0.1]
    return q


def occupancy(name):
    if name == "spheres":
        return synthetic.make_occupancy((24, 20, 28), "spheres", seed=4), 0.04
    if name == "dense":                                     # mostly filled: deep points, many leave the grid
        return synthetic.make_occupancy((7, 9, 11), "spheres", seed=4), 0.125
    if name == "corridor":                                  # two free cells between two walls
        occ = np.zeros((14, 6, 6), dtype=np.float32)
        occ[:6] = 1.0
        occ[8:] = 1.0
        return occ, 0.1
    if name == "flat_1x6x5":                                # degenerate axes of the interpolation and edge-gradient rules
        return (np.random.default_rng(1).random((1, 6, 5)) < 0.3).astype(np.float32), 0.04
    if name == "tiny_2x2x2":
        return (np.random.default_rng(1).random((2, 2, 2)) < 0.3).astype(np.float32), 0.04
    if name == "one_voxel":                                 # 5^3, the centre voxel filled
        occ = np.zeros((5, 5, 5), dtype=np.float32)
        occ[2, 2, 2] = 1.0
        return occ, 0.1
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def scene(name):
    """(sdf float32 read-only, resolution) of a named scene, computed once by the CPU oracle."""
    from oracle import oracle as O
    occ, res = occupancy(name)
    sdf, _, _ = O.sdf_from_occupancy(occ, res)
    sdf.setflags(write=False)
    return sdf, res


def queries(name):
    sdf, res = scene(name)
    if name == "corridor":                                  # 200 points inside the corridor
        rng = np.random.default_rng(3)
        lo = np.array([6.0, 0.0, 0.0]) * res
        return lo + rng.random((200, 3)) * (np.array([2.0, 6.0, 6.0]) * res)
    n = 4000 if name == "spheres" else 1500
    return query_cloud(sdf.shape, res, n, 11)


def frame_pair():
    """(grid_from_world 16 doubles column-major, rotation 9 doubles row-major) of an origin transform that is a rotation
    about z plus a translation, and world_from_grid as a 4x4 matrix."""
    c, s = np.cos(0.3), np.sin(0.3)
    world_from_grid = np.array([[c, -s, 0.0, 0.4], [s, c, 0.0, -0.2], [0.0, 0.0, 1.0, 0.05], [0.0, 0.0, 0.0, 1.0]])
    rotation = world_from_grid[:3, :3]
    grid_from_world = np.eye(4)
    grid_from_world[:3, :3] = rotation.T
    grid_from_world[:3, 3] = -(rotation.T @ world_from_grid[:3, 3])
    return grid_from_world.T.reshape(16).copy(), rotation.reshape(9).copy(), world_from_grid


def general_frame_pair():
    """The same three as frame_pair() for an origin transform whose rotation is about an axis that is none of x, y, z:
    (0.3, -0.5, 0.8) normalised, by 0.7 (Rodrigues' formula), so that every entry of `rotation` is far from 0 and +-1 and
    a transposed, dropped or swapped rotation changes every component; the same translation."""
    axis = np.array([0.3, -0.5, 0.8])
    axis /= np.linalg.norm(axis)
    k = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    rotation = np.eye(3) + np.sin(0.7) * k + (1.0 - np.cos(0.7)) * (k @ k)
    assert (np.abs(rotation) >= 0.05).all() and (np.abs(rotation) <= 0.95).all(), rotation
    world_from_grid = np.eye(4)
    world_from_grid[:3, :3] = rotation
    world_from_grid[:3, 3] = [0.4, -0.2, 0.05]
    grid_from_world = np.eye(4)
    grid_from_world[:3, :3] = rotation.T
    grid_from_world[:3, 3] = -(rotation.T @ world_from_grid[:3, 3])
    return grid_from_world.T.reshape(16).copy(), rotation.reshape(9).copy(), world_from_grid


def base_under(world_from_grid, world_from_base):
    """world_from_grid * world_from_base, both ways of writing a transform: a 4x4 matrix times 16 doubles column-major ->
    16 doubles column-major.  A tree on this base moves through the same part of the grid as before the frame."""
    base = np.asarray(world_from_base, dtype=np.float64).reshape(4, 4).T
    return (world_from_grid @ base).T.reshape(16).copy()


def to_world(points, world_from_grid):
    with np.errstate(invalid="ignore"):                     # (the cloud's NaN and infinite points)
        return points @ world_from_grid[:3, :3].T + world_from_grid[:3, 3]
