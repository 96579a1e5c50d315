"""Seeded inputs shared by tests/test_gpu_bodies.py (and read by tests/test_body_ref.py): the smallest shapes at which
vgt_hip_check_spheres can go wrong, with the answers of tests/body_ref.py computed once per case.

The grid is 12 x 10 x 9 at resolution 0.25, its field the CPU oracle's SDF of a few boxes (which the device's extraction
equals bit for bit, tests/test_gpu_sdf.py); every third case uses the same field with NaN and +-infinity cells, every
second one the same grid under an origin transform (rotated and shifted: tests/projection_cases.frame_pair).

The shapes (S spheres, L links, B configurations) cover every width of a configuration's lane segment (S = 1, 2, 3 -> 4,
31 / 32 -> 32, 33 / 63 / 64 -> 64), a partial last group of configurations, more than one slice of 64 spheres (65, 130),
a model larger than the kernel's LDS table (300 > 256), groups whose poses would fit the LDS budget of the kernel's
pose-staging variant (42 link poses per wave) and groups whose poses would not (S = 1 with L = 7: 448), and -- with the
launch limited to two workgroups, as tests/test_gpu_bodies.py does through the testing library -- more groups than the
waves of a launch take in one trip.

In every model: links in no order, radii of 0, a sphere at its link's origin (so that poses with a translation on the
cell lattice put a centre on cell faces, the grid's own faces included), and the last sphere a copy of the first (an exact
clearance tie, which the lower index must win).  In every batch of poses: centres inside and outside the grid, identity
rotations with translations on the lattice, a NaN and an infinite pose entry.  minimum_clearance is a clearance that
occurs in the case (the `<=` edge), and every second case sets the outside-is-collision flag.
"""
import collections
import functools

import numpy as np

import body_ref
import projection_cases

SHAPE = (12, 10, 9)
RESOLUTION = 0.25

# (S, L, B)
SHAPES = [
    (1, 1, 1), (1, 3, 67), (1, 7, 257), (2, 3, 2), (2, 1, 257), (3, 7, 5), (3, 3, 67), (31, 1, 2), (31, 7, 67),
    (32, 3, 5), (32, 1, 257), (33, 7, 1), (33, 3, 67), (63, 1, 5), (63, 7, 2), (64, 3, 67), (64, 1, 257), (65, 7, 1),
    (65, 3, 257), (130, 1, 2), (130, 7, 67), (130, 3, 257), (300, 3, 5), (300, 7, 67),
]

Case = collections.namedtuple(
    "Case", "name sdf resolution xyzr link poses minimum_clearance outside_is_collision grid_from_world rotation want")


@functools.lru_cache(maxsize=None)
def field(odd):
    """The scene's SDF (read-only); odd: with NaN and +-infinity cells, on a face of the grid and inside it."""
    from oracle import oracle as O
    occ = np.zeros(SHAPE, dtype=np.float32)
    occ[2:5, 1:4, 0:3] = 1.0
    occ[7:11, 5:9, 3:8] = 1.0
    occ[0:2, 7:10, 6:9] = 1.0
    occ[5, 5, 5] = 0.5
    sdf, _, _ = O.sdf_from_occupancy(occ, RESOLUTION)
    sdf = sdf.copy()
    if odd:
        sdf[6, 2, 4] = np.nan
        sdf[0, 0, 0] = np.nan
        sdf[9, 2, 2] = np.inf
        sdf[3, 8, 8] = -np.inf
        sdf[11, 9, 4] = np.inf
        sdf[5, 6, 1] = -np.inf
    sdf.setflags(write=False)
    return sdf


def model(num_spheres, num_links, seed):
    """(xyzr [S, 4], link [S] int32)"""
    rng = np.random.default_rng(seed)
    xyzr = np.empty((num_spheres, 4))
    xyzr[:, :3] = (rng.random((num_spheres, 3)) - 0.5) * 0.9
    xyzr[:, 3] = rng.random(num_spheres) * 0.3
    xyzr[::5, 3] = 0.0
    link = rng.integers(0, num_links, num_spheres).astype(np.int32)          # (in no order)
    xyzr[0, :3] = 0.0
    if num_spheres > 2:
        xyzr[-1] = xyzr[0]
        link[-1] = link[0]
    return xyzr, link


def poses(num_configurations, num_links, seed):
    """[B, L, 16] column-major world_from_link, in the grid's own frame"""
    rng = np.random.default_rng(seed)
    extent = np.array(SHAPE, dtype=np.float64) * RESOLUTION
    out = np.zeros((num_configurations, num_links, 16))
    for b in range(num_configurations):
        for k in range(num_links):
            q = rng.normal(size=4)
            q /= np.linalg.norm(q)
            w, x, y, z = q
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                          [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                          [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
            t = (rng.random(3) * 0.7 + 0.15) * extent
            if (b + k) % 4 == 3:                                             # some of it outside the grid
                t = (rng.random(3) * 1.3 - 0.15) * extent
            if (b + k) % 4 == 1:                                             # on the cell lattice, the grid's faces too
                R = np.eye(3)
                t = rng.integers(0, np.array(SHAPE) + 1).astype(np.float64) * RESOLUTION
            m = np.eye(4)
            m[:3, :3] = R
            m[:3, 3] = t
            out[b, k] = m.T.reshape(16)
    if num_configurations > 1:
        out[1, 0, 12] = np.nan
    if num_configurations > 3:
        out[3, num_links - 1, 0] = np.inf
    return out


@functools.lru_cache(maxsize=None)
def case(index):
    from oracle import oracle as O
    num_spheres, num_links, num_configurations = SHAPES[index]
    sdf = field(index % 3 == 2)
    xyzr, link = model(num_spheres, num_links, 100 + index)
    in_grid = poses(num_configurations, num_links, 200 + index)
    grid_from_world = rotation = None
    link_poses = in_grid
    if index % 2 == 1:
        grid_from_world, rotation, world_from_grid = projection_cases.frame_pair()
        with np.errstate(invalid="ignore"):
            m = in_grid.reshape(-1, 4, 4).transpose(0, 2, 1)
            link_poses = (world_from_grid @ m).transpose(0, 2, 1).reshape(in_grid.shape).copy()
    link_poses = link_poses.copy()
    link_poses[:, :, 3::4] = [7.0, -7.0, np.nan, 3.0]                        # (the row nobody reads)
    flag = index % 4 >= 2
    kw = dict(outside_is_collision=flag, grid_from_world=grid_from_world, rotation=rotation)
    first = body_ref.check_spheres(O, sdf, RESOLUTION, xyzr, link, link_poses, 0.0, **kw)
    finite = first.sphere_clearance[np.isfinite(first.sphere_clearance)]
    minimum_clearance = float(np.sort(finite)[len(finite) // 40]) if len(finite) else 0.0
    want = body_ref.check_spheres(O, sdf, RESOLUTION, xyzr, link, link_poses, minimum_clearance, **kw)
    for a in (xyzr, link, link_poses, *want):
        a.setflags(write=False)
    name = "S%d-L%d-B%d" % SHAPES[index]
    return Case(name, sdf, RESOLUTION, xyzr, link, link_poses, minimum_clearance, flag, grid_from_world, rotation, want)


def names():
    return ["S%d-L%d-B%d" % s for s in SHAPES]
