"""tests/motion_ref.py, the CPU restatement of vgt_hip_check_motions, held to answers derived by hand on a two-link tree;
the restatement under a turned grid against itself without one; and the shared cases of tests/motion_cases.py held to
what they must contain, so that no GPU test passes by accident.

The hand-made scene.  Field: 8 x 4 x 4 cells of resolution 1, sdf[x, y, z] = x + 1.5, so that the corrected centre
distance is x + 1 and the trilinear estimate at a point p with 0.5 <= p_x <= 7.5 is p_x + 0.5; the coarse gradient of an
inner cell is (1, 0, 0).  Tree: link 0 prismatic along x at (0, 1.5, 1.5), link 1 fixed on it at (1, 0, 0).  Sphere 0: on
link 1, radius 0.25 (clearance q + 1.25); sphere 1: on link 0, radius 0 (clearance q + 0.5, always the worst)."""
import numpy as np
import pytest

import body_ref
import kinematics_ref
import motion_cases as C
import motion_ref as R
from oracle import oracle as O


def scene():
    sdf = np.empty((8, 4, 4), dtype=np.float32)
    sdf[:] = (np.arange(8, dtype=np.float32) + 1.5)[:, None, None]
    origin0 = np.eye(4)
    origin0[:3, 3] = [0.0, 1.5, 1.5]
    origin1 = np.eye(4)
    origin1[:3, 3] = [1.0, 0.0, 0.0]
    tree = kinematics_ref.Tree([-1, 0], [kinematics_ref.PRISMATIC, kinematics_ref.FIXED], [0, 0],
                               [[1, 0, 0], [0, 0, 0]], [origin0.T.reshape(16), origin1.T.reshape(16)], 1)
    xyzr = np.array([[0.0, 0.0, 0.0, 0.25], [0.0, 0.0, 0.0, 0.0]])
    link = np.array([1, 0], dtype=np.int32)
    return sdf, tree, xyzr, link


def run(joint_from, joint_to, num_steps, **options):
    sdf, tree, xyzr, link = scene()
    return R.check_motions(O, sdf, 1.0, xyzr, link, tree, np.array(joint_from, dtype=np.float64).reshape(-1, 1),
                           np.array(joint_to, dtype=np.float64).reshape(-1, 1), num_steps, **options)


def test_interpolation_keeps_the_endpoints_bits():
    a = np.array([[0.1, -0.0], [3.0, np.nan]])
    b = np.array([[0.7, 5.0], [np.nan, np.nan]])
    q, first = R.interpolate(a, b, [3, 0])
    assert first.tolist() == [0, 4, 5]
    assert q[0].tobytes() == a[0].tobytes() and q[3].tobytes() == b[0].tobytes()
    assert q[1, 0] == 0.1 + (1.0 / 3.0) * (0.7 - 0.1) and q[2, 1] == -0.0 + (2.0 / 3.0) * (5.0 - -0.0)
    assert q[4].tobytes() == a[1].tobytes()                                          # n == 0: joint_to is not read
    q, _ = R.interpolate(a[:1], b[:1], 1)
    assert q.tobytes() == np.concatenate([a[:1], b[:1]]).tobytes()                   # n == 1: the two endpoints, no t


def test_a_motion_into_collision():
    # q = 5, 4, 3, 2, 1: clearances 5.5, 4.5, 3.5, 2.5, 1.5 (sphere 1)
    got = run([5.0], [1.0], 4, minimum_clearance=3.5)
    assert (got.status[0], got.first_collision[0], got.min_sample[0], got.min_sphere[0]) == (R.COLLISION, 2, 4, 1)
    assert got.min_clearance[0] == 1.5 and got.min_gradient[0].tolist() == [1.0, 0.0, 0.0] and got.fk_status[0] == 0
    stopped = run([5.0], [1.0], 4, minimum_clearance=3.5, stop_at_collision=True)
    assert (stopped.status[0], stopped.first_collision[0], stopped.min_sample[0]) == (R.COLLISION, 2, 2)
    assert stopped.min_clearance[0] == 3.5                                           # (the `<=` edge)
    clear = run([5.0], [1.0], 4, minimum_clearance=1.0, stop_at_collision=True)
    assert (clear.status[0], clear.first_collision[0], clear.min_sample[0]) == (R.CLEAR, -1, 4)
    assert clear.min_clearance[0] == 1.5


def test_ties_go_to_the_lowest_sample():
    # out and back through the same values would need two motions; a motion that goes nowhere ties on every sample
    got = run([3.0], [3.0], 5)
    assert (got.status[0], got.min_sample[0], got.min_clearance[0]) == (R.CLEAR, 0, 3.5)


def test_samples_without_a_value():
    # q = 5, 10, 15, 20: from k = 1 on both spheres are outside the grid
    got = run([5.0], [20.0], 3)
    assert (got.status[0], got.first_collision[0], got.min_sample[0], got.min_clearance[0]) == (R.NO_VALUE, -1, 0, 5.5)
    outside = run([5.0], [20.0], 3, outside_is_collision=True)
    assert (outside.status[0], outside.first_collision[0]) == (R.COLLISION, 1)
    nowhere = run([20.0], [30.0], 2)
    assert (nowhere.status[0], nowhere.min_sample[0], nowhere.min_sphere[0]) == (R.NO_VALUE, -1, -1)
    assert np.isnan(nowhere.min_clearance[0]) and np.isnan(nowhere.min_gradient[0]).all()


def test_fk_status_is_the_or_of_the_considered_samples():
    limits = np.array([[0.0, 6.0]])
    got = run([5.0, 5.0, 5.0], [np.inf, 7.0, 1.0], [2, 2, 0], joint_limits=limits)
    assert got.fk_status.tolist() == [3, 2, 0]                                       # inf: not computable and beyond 6
    assert got.status.tolist() == [R.NO_VALUE, R.CLEAR, R.CLEAR]
    stopped = run([5.0], [7.0], 2, joint_limits=limits, minimum_clearance=5.5, stop_at_collision=True)
    assert (stopped.first_collision[0], stopped.fk_status[0]) == (0, 0)              # (the later samples do not exist)


def test_one_sample_when_there_are_no_steps():
    got = run([2.0], [np.nan], 0)
    assert (got.status[0], got.min_sample[0], got.min_clearance[0], got.fk_status[0]) == (R.CLEAR, 0, 2.5, 0)


def threshold_off_every_clearance(clearances, quantile):
    """A minimum_clearance midway between two neighbouring distinct clearances that occur, at the quantile of the sorted
    distinct finite values (the first pair from there on that is further apart than 1e-6, so that the rounding of two more
    transforms, 1e-15, puts no sample on the other side); with one value only, 0.01 above it."""
    values = np.unique(clearances[np.isfinite(clearances)])
    if len(values) == 1:
        return float(values[0]) + 0.01
    at = int(quantile * (len(values) - 1))
    while values[at + 1] - values[at] <= 1e-6:
        at += 1
    return float((values[at] + values[at + 1]) * 0.5)


@pytest.mark.parametrize("index", [i for i in range(len(C.CASES)) if i not in C.FRAMED],
                         ids=[n for i, n in enumerate(C.names()) if i not in C.FRAMED])
def test_the_restatement_under_a_turned_grid(index):
    """The restatement under tests/projection_cases.general_frame_pair(), held to itself without a frame: the grid turned
    and shifted and the tree with it (world_from_grid * world_from_base) is the same scene.  With a threshold that no
    sample's clearance sits on, every integer output of every motion is equal with and without the stop flag,
    min_clearance agrees within 1e-9 and min_gradient is the plain one turned into the world (g * rotation^T for a row
    vector g) within 1e-12.  No motion is left out.  (With the cases' own threshold, a clearance that occurs, a sample on
    the `<=` edge may legitimately change sides under rounding.)"""
    import projection_cases
    case = C.case(index)
    assert case.grid_from_world is None and case.rotation is None
    grid_from_world, rotation, world_from_grid = projection_cases.general_frame_pair()
    base = projection_cases.base_under(world_from_grid, case.world_from_base)
    tree_name, num_spheres, odd, quantile, outside = C.CASES[index]
    threshold = threshold_off_every_clearance(case.samples.min_clearance, quantile)
    q, first = R.interpolate(case.joint_from, case.joint_to, case.num_steps)
    assert np.array_equal(first, case.first)
    plain = R.check_samples(O, case.sdf, C.RESOLUTION, case.xyzr, case.link, case.tree, q, threshold, outside, None, None,
                            case.world_from_base, case.joint_limits)
    turned = R.check_samples(O, case.sdf, C.RESOLUTION, case.xyzr, case.link, case.tree, q, threshold, outside,
                             grid_from_world, rotation, base, case.joint_limits)
    assert (plain.status == body_ref.COLLISION).any()
    r = rotation.reshape(3, 3)
    worst = [0.0, 0.0]
    for stop in (False, True):
        want, got = R.reduce_motions(plain, first, stop), R.reduce_motions(turned, first, stop)
        for field in ("status", "first_collision", "min_sample", "min_sphere", "fk_status"):
            assert np.array_equal(getattr(got, field), getattr(want, field)), field
        nan = np.isnan(want.min_clearance)
        assert np.array_equal(np.isnan(got.min_clearance), nan)
        infinite = np.isinf(want.min_clearance)
        assert np.array_equal(got.min_clearance[infinite], want.min_clearance[infinite])
        finite = ~nan & ~infinite
        if finite.any():
            worst[0] = max(worst[0], float(np.abs(got.min_clearance[finite] - want.min_clearance[finite]).max()))
        with np.errstate(invalid="ignore", over="ignore"):
            g = want.min_gradient
            rotated = np.stack([(g[:, 0] * r[i, 0] + g[:, 1] * r[i, 1]) + g[:, 2] * r[i, 2] for i in range(3)], axis=-1)
        same_kind = np.isfinite(rotated)
        assert np.array_equal(np.isfinite(got.min_gradient), same_kind)
        assert np.array_equal(np.isnan(got.min_gradient), np.isnan(rotated))
        assert np.array_equal(got.min_gradient[np.isinf(rotated)], rotated[np.isinf(rotated)])
        if same_kind.any():
            worst[1] = max(worst[1], float(np.abs(got.min_gradient[same_kind] - rotated[same_kind]).max()))
    print(case.name, "threshold", threshold, "largest differences: min_clearance %g, turned gradients %g" % tuple(worst))
    assert worst[0] <= 1e-9 and worst[1] <= 1e-12


def test_the_shared_cases_cover_what_the_gpu_tests_rely_on():
    seen = set()
    for index in range(len(C.CASES)):
        case = C.case(index)
        want, stopped = case.want, case.want_stopped
        steps = np.diff(case.first) - 1
        first = want.first_collision
        print(case.name, "statuses", np.bincount(want.status, minlength=3).tolist(), "minimum_clearance",
              case.minimum_clearance)
        assert np.array_equal(first, stopped.first_collision) and np.array_equal(want.status == R.COLLISION, first >= 0)
        seen |= {"status %d" % s for s in want.status.tolist()}
        for name, found in (("inside", (first > 0) & (first < steps)), ("late", first >= 64), ("at once", first == 0),
                            ("at the end", (first == steps) & (steps > 0)), ("late minimum", want.min_sample >= 64),
                            ("stop changes the minimum", want.min_sample != stopped.min_sample),
                            ("not computable", (want.fk_status & 1) != 0), ("limits", (want.fk_status & 2) != 0),
                            ("samples without a value", want.status == R.NO_VALUE)):
            if found.any():
                seen.add(name)
        # minimum_clearance is a clearance that occurs
        assert (case.samples.min_clearance == case.minimum_clearance).any()
        assert (case.samples.status == body_ref.COLLISION).any()
    assert seen >= {"status 0", "status 1", "status 2", "inside", "late", "at once", "at the end", "late minimum",
                    "stop changes the minimum", "not computable", "limits"}, seen
