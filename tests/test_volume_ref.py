"""(not gpu) tests/volume_ref.py, the restatement of vgt_hip_rasterize_spheres and vgt_hip_spheres_cover_points, against
answers derived by hand; and the conditions tests/volume_cases.py sets on the shared inputs."""
import numpy as np

import volume_cases as C
import volume_ref as R

RES = 0.25
SHAPE = (8, 9, 10)
CELL = (3, 4, 5)
CENTRE = [(3 + 0.5) * RES, (4 + 0.5) * RES, (5 + 0.5) * RES]        # 0.875, 1.125, 1.375: exact
NEIGHBOURS = [(2, 4, 5), (4, 4, 5), (3, 3, 5), (3, 5, 5), (3, 4, 4), (3, 4, 6)]


def pose(x=0.0, y=0.0, z=0.0):
    m = np.eye(4)
    m[:3, 3] = [x, y, z]
    return m.T.reshape(16)


def one_sphere(radius, centre=CENTRE, padding=0.0, **kw):
    """A sphere at its link's origin, the link at `centre`."""
    return R.rasterize_spheres(SHAPE, RES, [[0.0, 0.0, 0.0, radius]], [0], pose(*centre).reshape(1, 1, 16), padding, **kw)


def covered_cells(first):
    return sorted(map(tuple, np.argwhere(first >= 0).tolist()))


def test_radius_zero_covers_exactly_the_cell_whose_centre_it_is_on():
    first = one_sphere(0.0)
    assert first.dtype == np.int32 and first.shape == SHAPE
    assert covered_cells(first) == [CELL] and first[CELL] == 0


def test_the_tie_edge_covers_the_six_face_neighbours():
    """R = 0.25 exactly: d^2 == R^2 == 0.0625 for the face neighbours, and `<=` covers them; nothing else is that near."""
    assert covered_cells(one_sphere(0.25)) == sorted([CELL] + NEIGHBOURS)
    # the same R from radius + padding, both ways round
    assert covered_cells(one_sphere(0.125, padding=0.125)) == sorted([CELL] + NEIGHBOURS)
    assert covered_cells(one_sphere(0.5, padding=-0.25)) == sorted([CELL] + NEIGHBOURS)


def test_just_below_the_tie_only_the_one_cell():
    assert covered_cells(one_sphere(float(np.nextafter(0.25, 0)))) == [CELL]


def test_a_centre_on_a_lattice_corner_with_radius_zero_covers_nothing():
    assert covered_cells(one_sphere(0.0, centre=[0.75, 1.0, 1.25])) == []


def test_two_configurations_on_one_cell_give_the_lower_index():
    poses = np.stack([pose(*CENTRE), pose(*CENTRE), pose(0.125, 0.125, 0.125)]).reshape(3, 1, 16)
    first = R.rasterize_spheres(SHAPE, RES, [[0.0, 0.0, 0.0, 0.0]], [0], poses)
    assert first[CELL] == 0 and first[0, 0, 0] == 2 and (first >= 0).sum() == 2
    first = R.rasterize_spheres(SHAPE, RES, [[0.0, 0.0, 0.0, 0.0]], [0], poses[::-1].copy())
    assert first[CELL] == 1 and first[0, 0, 0] == 0


def test_base_and_keep_merge_as_unsigned_minima_in_either_order():
    poses = np.stack([pose(*CENTRE), pose(0.125, 0.125, 0.125), pose(*CENTRE), pose(0.375, 0.125, 0.125)])
    poses = poses.reshape(4, 1, 16)
    model = ([[0.0, 0.0, 0.0, 0.0]], [0])
    whole = R.rasterize_spheres(SHAPE, RES, *model, poses, base=10)
    assert whole[CELL] == 10 and whole[0, 0, 0] == 11 and whole[1, 0, 0] == 13 and (whole >= 0).sum() == 3
    low_first = R.rasterize_spheres(SHAPE, RES, *model, poses[:2], base=10)
    low_first = R.rasterize_spheres(SHAPE, RES, *model, poses[2:], base=12, into=low_first)
    high_first = R.rasterize_spheres(SHAPE, RES, *model, poses[2:], base=12)
    assert high_first[CELL] == 12 and high_first[0, 0, 0] == -1                   # (-1 is the greatest unsigned value)
    high_first = R.rasterize_spheres(SHAPE, RES, *model, poses[:2], base=10, into=high_first)
    assert np.array_equal(low_first, whole) and np.array_equal(high_first, whole)


def test_what_is_not_usable_covers_nothing():
    assert covered_cells(one_sphere(0.25, padding=-0.3)) == []                       # R < 0
    assert covered_cells(one_sphere(0.25, padding=-0.25)) == [CELL]                  # R == 0
    for entry, value in ((12, np.nan), (13, np.inf), (0, -np.inf), (5, np.nan)):
        m = pose(*CENTRE)
        m[entry] = value
        got = R.rasterize_spheres(SHAPE, RES, [[0.1, 0.1, 0.1, 5.0]], [0], m.reshape(1, 1, 16))
        assert covered_cells(got) == [], entry
    m = pose(*CENTRE)
    m[3] = np.nan                                                                    # (the row nobody reads)
    assert (R.rasterize_spheres(SHAPE, RES, [[0.1, 0.1, 0.1, 5.0]], [0], m.reshape(1, 1, 16)) == 0).all()
    for link in (1, -1, 2 ** 31 - 1):
        got = R.rasterize_spheres(SHAPE, RES, [[0.0, 0.0, 0.0, 5.0]], [link], pose(*CENTRE).reshape(1, 1, 16))
        assert covered_cells(got) == [], link
    # a grid_from_world that makes the centre infinite
    M = np.eye(4).T.reshape(16).copy()
    M[12] = np.inf
    assert covered_cells(one_sphere(5.0, grid_from_world=M)) == []
    # nothing to cover with
    assert (R.rasterize_spheres(SHAPE, RES, np.zeros((0, 4)), [], np.zeros((3, 1, 16))) == -1).all()
    assert (R.rasterize_spheres(SHAPE, RES, [[0, 0, 0, 9.0]], [0], np.zeros((0, 1, 16))) == -1).all()


def test_grid_from_world_moves_the_centre():
    M = pose(-1.0, 0.0, 0.25)                                                        # c = w + (-1, 0, 0.25)
    first = one_sphere(0.0, centre=[CENTRE[0] + 1.0, CENTRE[1], CENTRE[2] - 0.25], grid_from_world=M)
    assert covered_cells(first) == [CELL]


def test_points_first_configuration_first_sphere_and_filtered_bits():
    xyzr = [[0.0, 0.0, 0.0, 0.25], [0.0, 0.0, 0.0, 1.0], [0.5, 0.0, 0.0, 0.0]]
    link = [0, 1, 0]
    poses = np.stack([pose(1, 1, 1), pose(9, 9, 9), pose(3, 3, 3), pose(1, 1, 1)]).reshape(2, 2, 16)
    points = np.array([[1.0, 1.0, 1.25],        # b 0: on sphere 0's surface (tie); b 1 sphere 1 covers too: (0, 0)
                       [1.0, 1.5, 1.0],         # b 0: none; b 1: sphere 1 at (1, 1, 1) with R = 1: (1, 1)
                       [1.5, 1.0, 1.0],         # b 0: sphere 2 (R = 0) equals its centre: (0, 2)
                       [-0.0, 5.0, -3.0],       # nothing
                       [np.nan, 1.0, 1.0], [1.0, np.inf, 1.0], [1.0, 1.0, -np.inf],
                       [3.5, 3.0, 3.0]],        # b 1: sphere 1 would cover (d = 2.69 > 1: no); sphere 2 at (3.5, 3, 3): (1, 2)
                      dtype=np.float32)
    got = R.spheres_cover_points(points, xyzr, link, poses)
    assert got.first_configuration.tolist() == [0, 1, 0, -1, -1, -1, -1, 1]
    assert got.first_sphere.tolist() == [0, 1, 2, -1, -1, -1, -1, 2]
    assert got.first_configuration.dtype == np.int32 and got.filtered.dtype == np.float32
    kept = got.first_configuration < 0
    assert np.array_equal(got.filtered[kept].view(np.uint32), points[kept].view(np.uint32))  # -0.0, NaN, inf as they are
    assert got.filtered[3].view(np.uint32)[0] == 0x80000000
    assert np.isnan(got.filtered[~kept]).all()
    # padding and a world_from_points: the cloud shifted by (-1, 0, 0) and the transform shifting it back
    shifted = points - np.array([1.0, 0.0, 0.0], dtype=np.float32)
    moved = R.spheres_cover_points(shifted, xyzr, link, poses, world_from_points=pose(1.0, 0.0, 0.0))
    assert np.array_equal(moved.first_configuration, got.first_configuration)
    assert np.array_equal(moved.first_sphere, got.first_sphere)
    padded = R.spheres_cover_points(points, xyzr, link, poses, padding=-0.25)      # sphere 0: R = 0; sphere 2: not usable
    assert padded.first_configuration.tolist() == [1, 1, 1, -1, -1, -1, -1, -1]
    # a transform with a non-finite entry: q is not finite, nothing is covered
    T = pose()
    T[12] = np.nan
    assert (R.spheres_cover_points(points, xyzr, link, poses, world_from_points=T).first_configuration == -1).all()
    empty = R.spheres_cover_points(np.zeros((0, 3), np.float32), xyzr, link, poses)
    assert [len(a) for a in empty] == [0, 0, 0]


def test_grid_and_point_forms_agree_on_cell_centres():
    c = C.case(4)
    points = R.cell_centres(c.shape, c.resolution).reshape(-1, 3).astype(np.float32)   # exact at this resolution
    assert np.array_equal(points.astype(np.float64), R.cell_centres(c.shape, c.resolution).reshape(-1, 3))
    got = R.spheres_cover_points(points, c.xyzr, c.link, c.poses, c.padding)
    assert c.grid_from_world is None and np.array_equal(got.first_configuration, c.want.reshape(-1))


def test_the_shared_cases_cover_something_and_not_everything():
    print(C.check_conditions())
