"""(not gpu) tests/body_ref.py, the CPU restatement of vgt_hip_check_spheres, against answers derived by hand on a
4 x 4 x 4 field at resolution 1 whose value is the cell's x index: at the centre of cell (i, j, k) the trilinear estimate
is the corrected centre distance i - 0.5 (for i >= 0.5; cell 0 holds 0, corrected to -0.5), and the coarse gradient is
(1, 0, 0) everywhere (central differences inside, one-sided ones on the faces).  Every status, the tie rule, the `<=`
edge, the flag, an all-outside configuration, column-major poses, both transforms, non-finite cells and a link out of
range; and the shared cases of tests/body_cases.py hold what their docstring promises."""
import numpy as np
import pytest

import body_cases as C
import body_ref as R
from oracle import oracle as O

NAN = np.nan


def ramp():
    return np.broadcast_to(np.arange(4, dtype=np.float32)[:, None, None], (4, 4, 4)).copy()


def translation(x, y, z):
    m = np.eye(4)
    m[:3, 3] = [x, y, z]
    return m.T.reshape(16)                                                        # column-major


# sphere 0: link 0, radius 0.25;  sphere 1: link 1, radius 0;  sphere 2: a copy of sphere 0
XYZR = np.array([[0.0, 0.0, 0.0, 0.25], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.25]])
LINK = np.array([0, 1, 0], dtype=np.int32)
INSIDE = np.stack([translation(1.5, 1.5, 1.5), translation(2.5, 1.5, 1.5)])       # clearances 0.25, 1.5, 0.25
HALF_OUT = np.stack([translation(-1.0, 1.5, 1.5), translation(3.5, 0.5, 0.5)])    # -, 2.5, -
ALL_OUT = np.stack([translation(1.5, 4.5, 1.5), translation(1.5, 1.5, -0.5)])     # -, -, -
POSES = np.stack([INSIDE, HALF_OUT, ALL_OUT])


def test_statuses_counts_and_the_tie_rule():
    got = R.check_spheres(O, ramp(), 1.0, XYZR, LINK, POSES, minimum_clearance=0.0)
    assert got.status.tolist() == [R.CLEAR, R.CLEAR, R.NO_VALUE] and got.status.dtype == np.uint8
    assert got.num_below.tolist() == [0, 0, 0] and got.num_outside.tolist() == [0, 2, 3]
    assert got.min_sphere.tolist() == [0, 1, -1] and got.min_sphere.dtype == np.int32     # (0, not its copy 2)
    assert np.array_equal(got.min_clearance, [0.25, 2.5, NAN], equal_nan=True)
    assert np.array_equal(got.min_gradient, [[1, 0, 0], [1, 0, 0], [NAN] * 3], equal_nan=True)
    assert np.array_equal(got.sphere_clearance, [[0.25, 1.5, 0.25], [NAN, 2.5, NAN], [NAN] * 3], equal_nan=True)
    assert np.array_equal(got.sphere_gradient[0], [[1, 0, 0]] * 3)
    assert np.isnan(got.sphere_gradient[2]).all() and np.isnan(got.sphere_gradient[1, 0]).all()


def test_the_comparison_is_less_or_equal_and_the_flag_counts_outside_spheres():
    got = R.check_spheres(O, ramp(), 1.0, XYZR, LINK, POSES, minimum_clearance=0.25)
    assert got.status.tolist() == [R.COLLISION, R.CLEAR, R.NO_VALUE] and got.num_below.tolist() == [2, 0, 0]
    got = R.check_spheres(O, ramp(), 1.0, XYZR, LINK, POSES, minimum_clearance=np.nextafter(0.25, 0.0))
    assert got.status.tolist() == [R.CLEAR, R.CLEAR, R.NO_VALUE] and got.num_below.tolist() == [0, 0, 0]
    got = R.check_spheres(O, ramp(), 1.0, XYZR, LINK, POSES, minimum_clearance=0.0, outside_is_collision=True)
    assert got.status.tolist() == [R.CLEAR, R.COLLISION, R.COLLISION]
    assert got.min_sphere.tolist() == [0, 1, -1] and got.num_outside.tolist() == [0, 2, 3]   # (the rest is unchanged)
    got = R.check_spheres(O, ramp(), 1.0, XYZR, LINK, POSES, minimum_clearance=np.inf)
    assert got.num_below.tolist() == [3, 1, 0]


def test_poses_are_column_major_and_only_twelve_entries_are_read():
    # a quarter turn about z: the link's x axis is the world's y axis
    m = np.array([[0.0, -1.0, 0.0, 0.5], [1.0, 0.0, 0.0, 0.5], [0.0, 0.0, 1.0, 0.5], [9.0, NAN, np.inf, -3.0]])
    xyzr = np.array([[2.0, -1.0, 1.0, 0.5]])                                      # -> (1.5, 2.5, 1.5): cell (1, 2, 1)
    w, ok = R.world_centres(xyzr, [0], m.T.reshape(1, 1, 16))
    assert ok.all() and np.array_equal(w, [[[1.5, 2.5, 1.5]]])
    got = R.check_spheres(O, ramp(), 1.0, xyzr, [0], m.T.reshape(1, 1, 16))
    assert got.status.tolist() == [R.COLLISION] and np.array_equal(got.min_clearance, [0.0])
    # the 4 x 4 form of the binding is the transpose of that memory
    assert np.array_equal(m[None, None].transpose(0, 1, 3, 2).reshape(1, 1, 16), m.T.reshape(1, 1, 16),
                          equal_nan=True)


def test_both_transforms():
    # the grid's origin at (10, 20, 30) in the world, turned a quarter about z: world = Rz * grid + t
    rotation = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    t = np.array([10.0, 20.0, 30.0])
    grid_from_world = np.eye(4)
    grid_from_world[:3, :3] = rotation.T
    grid_from_world[:3, 3] = -(rotation.T @ t)
    centre = rotation @ np.array([2.5, 0.5, 3.5]) + t                             # the centre of cell (2, 0, 3)
    got = R.check_spheres(O, ramp(), 1.0, [[0.0, 0.0, 0.0, 0.5]], [0], translation(*centre).reshape(1, 1, 16),
                          grid_from_world=grid_from_world.T.reshape(16), rotation=rotation.reshape(9))
    assert got.status.tolist() == [R.CLEAR] and np.array_equal(got.min_clearance, [1.0])
    assert np.array_equal(got.min_gradient, [[0.0, 1.0, 0.0]])                    # the grid's x is the world's y


def test_non_finite_cells_and_poses():
    field = ramp()
    field[1, 1, 1] = NAN
    field[2, 2, 2] = -np.inf
    field[3, 0, 0] = np.inf
    xyzr = np.zeros((1, 4))
    poses = np.stack([translation(1.5, 1.5, 1.5), translation(2.5, 2.5, 2.5), translation(3.5, 0.5, 0.5),
                      translation(NAN, 1.5, 1.5), translation(np.inf, 1.5, 1.5)]).reshape(5, 1, 16)
    got = R.check_spheres(O, field, 1.0, xyzr, [0], poses, outside_is_collision=False)
    # a NaN clearance has a value, is never below and is no candidate; -inf is below and the least; +inf is a candidate
    assert got.status.tolist() == [R.NO_VALUE, R.COLLISION, R.CLEAR, R.NO_VALUE, R.NO_VALUE]
    assert got.num_outside.tolist() == [0, 0, 0, 1, 1] and got.num_below.tolist() == [0, 1, 0, 0, 0]
    assert got.min_sphere.tolist() == [-1, 0, 0, -1, -1]
    assert np.array_equal(got.min_clearance, [NAN, -np.inf, np.inf, NAN, NAN], equal_nan=True)
    assert np.isnan(got.sphere_clearance[0, 0]) and not np.isnan(got.sphere_gradient[0, 0]).any()
    flagged = R.check_spheres(O, field, 1.0, xyzr, [0], poses, outside_is_collision=True)
    assert flagged.status.tolist() == [R.NO_VALUE, R.COLLISION, R.CLEAR, R.COLLISION, R.COLLISION]


def test_a_link_out_of_range_is_a_sphere_without_a_value():
    got = R.check_spheres(O, ramp(), 1.0, XYZR, [0, 2, -1], POSES[:1])
    assert got.num_outside.tolist() == [2] and got.min_sphere.tolist() == [0] and got.status.tolist() == [R.CLEAR]
    assert np.array_equal(got.sphere_clearance, [[0.25, NAN, NAN]], equal_nan=True)


def test_nothing_to_compare():
    none = R.check_spheres(O, ramp(), 1.0, np.zeros((0, 4)), np.zeros(0, np.int32), np.zeros((3, 2, 16)))
    assert none.status.tolist() == [R.NO_VALUE] * 3 and none.min_sphere.tolist() == [-1] * 3
    assert none.num_outside.tolist() == [0] * 3 and none.sphere_clearance.shape == (3, 0)
    empty = R.check_spheres(O, np.zeros((4, 0, 4), np.float32), 1.0, XYZR, LINK, POSES)
    assert empty.status.tolist() == [R.NO_VALUE] * 3 and empty.num_outside.tolist() == [3] * 3
    assert np.isnan(empty.min_clearance).all() and np.isnan(empty.sphere_gradient).all()
    no_configurations = R.check_spheres(O, ramp(), 1.0, XYZR, LINK, np.zeros((0, 2, 16)))
    assert no_configurations.status.shape == (0,) and no_configurations.sphere_gradient.shape == (0, 3, 3)


@pytest.mark.parametrize("index", range(len(C.SHAPES)), ids=C.names())
def test_shared_cases_hold_what_they_promise(index):
    case = C.case(index)
    want = case.want
    s, links, b = C.SHAPES[index]
    assert case.xyzr.shape == (s, 4) and case.poses.shape == (b, links, 16) and want.sphere_clearance.shape == (b, s)
    assert (case.xyzr[:, 3] == 0.0).any() and (case.xyzr[:, 3] >= 0.0).all()
    assert np.count_nonzero(want.sphere_clearance == case.minimum_clearance) >= 1          # the `<=` edge occurs
    if s > 2:
        assert np.array_equal(case.xyzr[0], case.xyzr[-1]) and (want.min_sphere != s - 1).all()   # the tie's loser
    if links > 1 and s > 8:
        assert (np.diff(case.link) < 0).any()
    if b > 3:
        assert np.isnan(case.poses).any() and np.isinf(case.poses).any()
    if b >= 67:
        assert (want.num_outside > 0).any() and (want.num_below > 0).any()
        assert R.COLLISION in want.status and (s > 130 or R.CLEAR in want.status)


def test_shared_cases_cover_every_status_and_odd_values():
    seen = set()
    odd = 0
    for index in range(len(C.SHAPES)):
        want = C.case(index).want
        seen |= set(want.status.tolist())
        has = ~np.isnan(want.sphere_gradient).all(axis=2)
        odd += np.count_nonzero(np.isnan(want.sphere_clearance) & has) + np.count_nonzero(np.isinf(want.sphere_clearance))
    assert seen == {R.CLEAR, R.COLLISION, R.NO_VALUE} and odd > 100
