"""Seeded inputs shared by tests/test_gpu_volumes.py (and read by tests/test_volume_ref.py): the smallest shapes at which
vgt_hip_rasterize_spheres and vgt_hip_spheres_cover_points can go wrong, with the answers of tests/volume_ref.py
computed once per case.

The grid is 24 x 21 x 19 at resolution 0.25 (9576 cells, no extent a multiple of 8 or 64).  The models are
body_cases.model(S, L, seed): links in no order, radii of 0, a sphere at its link's origin, the last sphere a copy of the
first.  The poses are built the way body_cases.poses builds them, laid over this grid's extent: random rotations,
translations on the cell lattice, some outside the grid, a NaN and an infinite entry, the row nobody reads filled with
junk.  Every second case is under projection_cases.frame_pair().  The shapes are the 24 (S, L, B) of body_cases.SHAPES:
S = 1 ... 300 (beyond the rasterizer's LDS table and the point kernel's chunk, both 256), B = 1 ... 257, and -- with the
launches limited to two workgroups, as tests/test_gpu_volumes.py does through the testing library -- persistent waves
and workgroups that take several trips.  Padding alternates between 0.0, 0.1 and -0.05 (which makes some R negative).

Every third grid case (those with padding 0.0) gets two more spheres on link 0, S + 2 in all, and its last
configuration an identity pose of link 0 on the lattice: one sphere centred exactly on the centre of cell (5, 6, 7) with a
radius of exactly two cells (the `<=` tie: in the cases without a frame the six cells two steps along an axis are
covered by d^2 == R^2 alone), and one at 0.05 from the grid's corner with radius 0.4, whose box hangs over that corner.

Point cases: N in {1, 63, 64, 65, 257, 1000}, twice each, over the models and (world) poses of a grid case.  Half the
points are drawn near sphere centres, a few lie exactly on a centre (sphere 0 sits at its link's origin with radius 0, so
on a lattice pose with padding 0 only the point that EQUALS the centre is covered), a few carry NaN or +-inf
coordinates; half the cases are under a world_from_points.

check_conditions() asserts what the inputs must satisfy so that no test passes by covering nothing.
"""
import collections
import functools

import numpy as np

import body_cases
import projection_cases
import volume_ref

SHAPE = (24, 21, 19)
RESOLUTION = 0.25
SHAPES = body_cases.SHAPES
PADDINGS = (0.0, 0.1, -0.05)
TIE_CELL = (5, 6, 7)

# (N, index of the grid case whose model and poses the cloud is tested against)
POINT_CASES = [(1, 5), (63, 3), (64, 8), (65, 12), (257, 15), (1000, 23), (1, 20), (63, 22), (64, 1), (65, 18), (257, 10),
               (1000, 21)]

GridCase = collections.namedtuple("GridCase", "name shape resolution xyzr link poses padding grid_from_world want")
PointCase = collections.namedtuple("PointCase", "name points xyzr link poses padding world_from_points want")


def poses(num_configurations, num_links, seed):
    """[B, L, 16] column-major world_from_link in the grid's own frame: body_cases.poses over this grid's extent"""
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


def names():
    return ["S%d-L%d-B%d" % s for s in SHAPES]


def has_extra_spheres(index):
    return index % 3 == 0


@functools.lru_cache(maxsize=None)
def inputs(index):
    """(xyzr, link, link_poses, padding, grid_from_world) of grid case `index`, read-only"""
    num_spheres, num_links, num_configurations = SHAPES[index]
    xyzr, link = body_cases.model(num_spheres, num_links, 100 + index)
    in_grid = poses(num_configurations, num_links, 200 + index)
    padding = PADDINGS[index % 3]
    if has_extra_spheres(index):
        half = RESOLUTION / 2
        lattice = np.array(TIE_CELL, dtype=np.float64) * RESOLUTION
        tie = np.array([half, half, half, 2 * RESOLUTION])
        corner = np.concatenate([0.05 - lattice, [0.4]])
        xyzr = np.concatenate([xyzr, tie[None], corner[None]])
        link = np.concatenate([link, np.zeros(2, np.int32)])
        m = np.eye(4)
        m[:3, 3] = lattice
        in_grid[-1, 0] = m.T.reshape(16)
    grid_from_world = None
    link_poses = in_grid
    if index % 2 == 1:
        grid_from_world, _, world_from_grid = projection_cases.frame_pair()
        with np.errstate(invalid="ignore"):
            m = in_grid.reshape(-1, 4, 4).transpose(0, 2, 1)
            link_poses = (world_from_grid @ m).transpose(0, 2, 1).reshape(in_grid.shape).copy()
    link_poses = link_poses.copy()
    link_poses[:, :, 3::4] = [7.0, -7.0, np.nan, 3.0]                        # (the row nobody reads)
    for a in (xyzr, link, link_poses):
        a.setflags(write=False)
    return xyzr, link, link_poses, padding, grid_from_world


@functools.lru_cache(maxsize=None)
def case(index):
    xyzr, link, link_poses, padding, grid_from_world = inputs(index)
    want = volume_ref.rasterize_spheres(SHAPE, RESOLUTION, xyzr, link, link_poses, padding, 0, None, grid_from_world)
    want.setflags(write=False)
    return GridCase(names()[index], SHAPE, RESOLUTION, xyzr, link, link_poses, padding, grid_from_world, want)


def point_names():
    return ["N%d-%s" % (n, names()[index]) for n, index in POINT_CASES]


@functools.lru_cache(maxsize=None)
def point_case(number):
    num_points, index = POINT_CASES[number]
    xyzr, link, link_poses, padding, _ = inputs(index)
    rng = np.random.default_rng(300 + number)
    c, _, usable = volume_ref.usable_spheres(xyzr, link, link_poses, padding)
    extent = np.array(SHAPE, dtype=np.float64) * RESOLUTION
    world = (rng.random((num_points, 3)) * 1.2 - 0.1) * extent
    if index % 2 == 1:
        world = projection_cases.to_world(world, projection_cases.frame_pair()[2])
    pairs = np.argwhere(usable)
    if len(pairs):
        near = rng.random(num_points) < 0.5
        pick = pairs[rng.integers(0, len(pairs), num_points)]
        centres = c[pick[:, 0], pick[:, 1]]
        world[near] = centres[near] + rng.normal(size=(num_points, 3))[near] * 0.12
        # exactly on a centre; sphere 0 (radius 0, at its link's origin) first, whose centre on a lattice pose is a float32
        on_centre = np.argwhere(usable[:, 0])
        for k, i in enumerate(range(2, num_points, 23)):
            b, s = (on_centre[k % len(on_centre)][0], 0) if len(on_centre) and k % 2 == 0 else pick[i]
            world[i] = c[b, s]
    world_from_points = None
    points = world
    if number % 2 == 1:
        c3, s3 = np.cos(-0.7), np.sin(-0.7)
        T = np.array([[c3, 0.0, s3, 0.9], [0.0, 1.0, 0.0, -0.3], [-s3, 0.0, c3, 1.1], [0.0, 0.0, 0.0, 1.0]])
        world_from_points = T.T.reshape(16).copy()
        points = (world - T[:3, 3]) @ T[:3, :3]                              # R^T (w - t)
    points = points.astype(np.float32)
    for k, i in enumerate(range(7, num_points, 41)):
        points[i, k % 3] = [np.nan, np.inf, -np.inf][k % 3]
    want = volume_ref.spheres_cover_points(points, xyzr, link, link_poses, padding, world_from_points)
    for a in (points, *want):
        a.setflags(write=False)
    return PointCase(point_names()[number], points, xyzr, link, link_poses, padding, world_from_points, want)


@functools.lru_cache(maxsize=None)
def check_conditions():
    """What the inputs must satisfy, so that a test cannot pass by covering nothing; -> the figures, for printing."""
    shares, several, distinct = [], 0, []
    for index in range(len(SHAPES)):
        c = case(index)
        covered = c.want >= 0
        assert not covered.all(), c.name
        shares.append(float(covered.mean()))
        distinct.append(len(np.unique(c.want[covered])))
        # cells that two or more configurations cover: some cell is covered by a configuration above its first
        xyzr, link, link_poses, padding, grid_from_world = inputs(index)
        if distinct[-1] and link_poses.shape[0] > 1:
            first = int(c.want[covered].min())
            rest = volume_ref.rasterize_spheres(SHAPE, RESOLUTION, xyzr, link, link_poses[first + 1:], padding, first + 1,
                                                None, grid_from_world)
            several += bool(((rest >= 0) & (c.want == first)).any())
        if has_extra_spheres(index) and grid_from_world is None:
            b = link_poses.shape[0] - 1
            x, y, z = TIE_CELL
            for cell in ((x + 2, y, z), (x - 2, y, z), (x, y + 2, z), (x, y - 2, z), (x, y, z + 2), (x, y, z - 2)):
                assert 0 <= c.want[cell] <= b, (c.name, cell)                 # the `<=` tie covers it
            assert 0 <= c.want[0, 0, 0] <= b, c.name                          # the sphere over the corner
    assert sum(0.05 <= s <= 0.90 for s in shares) >= 12, shares
    assert several >= 8, several
    both = 0
    for number in range(len(POINT_CASES)):
        found = point_case(number).want.first_configuration >= 0
        both += bool(found.any() and not found.all())
    assert both >= len(POINT_CASES) // 2, both
    return dict(shares=[round(s, 3) for s in shares], several=several, distinct=distinct, point_cases_with_both=both)
