"""(not gpu) tests/ik_ref.py, the numpy restatement of vgt_hip_solve_ik, checked on its own: its columns against central
differences of tests/kinematics_ref.py, what a CONVERGED row promises, the share of problems that converge near the
truth, and the statuses of the planted rows of tests/ik_cases.py."""
import numpy as np
import pytest

import ik_cases as C
import ik_ref
import kinematics_ref as R


def _rotation(pose):
    return pose[[0, 1, 2, 4, 5, 6, 8, 9, 10]].reshape(3, 3).T


@pytest.mark.parametrize("name, tip", [("arm", 7), ("body", 13), ("serial-16", 17), ("serial-5", 6)])
def test_columns_are_the_derivative_of_the_tip(name, tip):
    """Central differences at h = 1e-6 on trees with unit axes: truncation is of order h^2 = 1e-12, rounding of order
    2^-53 / h = 1e-10, both far inside the 1e-7 (relative to the column's largest entry) asked here.  The rotational half
    is the vee of the skew part of R(q + h) R(q - h)^T over 2 h: sin(2 h |omega|) / (2 h) times the axis."""
    t = C.tree(name)
    assert tip == t.num_links - 1 or name == "body"
    rng = np.random.default_rng(5)
    q = (rng.random((3, t.num_joints)) * 2.0 - 1.0) * 2.0
    poses, _ = R.forward_kinematics(t, q)
    columns = ik_ref.columns(t, tip, poses, np.ones(6))
    moving = ik_ref.moving_links(t, tip)
    assert len(columns) == len(moving) > 0
    h = 1e-6
    worst = 0.0
    for c, i in zip(columns, moving):
        j = int(t.joint_index[i])
        up, down = q.copy(), q.copy()
        up[:, j] += h
        down[:, j] -= h
        a = R.forward_kinematics(t, up)[0][:, tip]
        b = R.forward_kinematics(t, down)[0][:, tip]
        for row in range(len(q)):
            skew = _rotation(a[row]) @ _rotation(b[row]).T
            numeric = np.concatenate([(a[row, 12:15] - b[row, 12:15]) / (2 * h),
                                      np.array([skew[2, 1] - skew[1, 2], skew[0, 2] - skew[2, 0],
                                                skew[1, 0] - skew[0, 1]]) / (4 * h)])
            stated = np.array([c[k][row] for k in range(6)])
            worst = max(worst, float(np.abs(numeric - stated).max() / np.abs(stated).max()))
    print(name, "moving links", len(moving), "largest relative difference", worst)
    assert worst <= 1e-7


@pytest.mark.parametrize("name", C.case_names())
def test_converged_rows_keep_their_promise(name):
    case = C.case(name)
    want = case.want
    done = want.status == ik_ref.CONVERGED
    poses, _ = R.forward_kinematics(case.tree, want.joints[done], case.world_from_base)
    assert np.array_equal(poses[:, case.tip].view(np.uint64), want.tip_pose[done].view(np.uint64))
    w = case.options["task_weights"] or (1,) * 6
    tolerance = [case.options["position_tolerance"]] * 3 + [case.options["rotation_tolerance"]] * 3
    for k in range(6):
        if w[k] != 0:
            assert (np.abs(want.error[done, k]) <= tolerance[k]).all()
    # the error is the one at the returned row, and the tip aims at target b / R
    aim = np.repeat(case.targets, case.seeds_per_target, axis=0)
    assert np.array_equal((aim[done, 12:15] - want.tip_pose[done, 12:15]).view(np.uint64),
                          want.error[done, :3].view(np.uint64))
    assert (want.iterations <= case.options["max_iterations"]).all()
    if case.joint_limits is not None:
        # (a NaN in a column off the chain is handed through, and compares false as in the forward kinematics' test)
        outside = (want.joints < case.joint_limits[:, 0]) | (want.joints > case.joint_limits[:, 1])
        assert np.array_equal(outside.any(axis=1), (want.fk_status & R.OUTSIDE_LIMITS) != 0)


def test_most_problems_near_the_truth_converge():
    """A condition on the definition, not a measurement: with seeds within 0.1 of a solution, at least 90 % of the
    problems converge (lambda = 0.01, K = 50, max_step 0.5, tolerances 1e-6); three planted rows cannot."""
    for name, spec in (("arm-near-200", ("arm", 7, 200, 1, 0.1, False, None, {})),
                       ("body13-near-200", ("body", 13, 200, 1, 0.1, False, None, {}))):
        t, tip, targets, per_target, seeds, _, base, limits, options = C.problem(name, spec)
        got = ik_ref.solve_ik(t, tip, targets, seeds, per_target, base, limits, **options)
        converged = int((got.status == ik_ref.CONVERGED).sum())
        print(name, "converged", converged, "of 200; median steps", float(np.median(got.iterations)))
        assert converged >= 180


def test_planted_rows():
    for name in ("arm-1.0-B257", "body13-near-B257", "serial-longest-B65"):
        case = C.case(name)
        want = case.want
        assert want.status[0] == ik_ref.CONVERGED and want.iterations[0] == 0
        assert np.array_equal(want.joints[0].view(np.uint64), case.seeds[0].view(np.uint64))
        # half a turn away: the cross products vanish at the seed, the trace says that it is no solution
        assert want.status[1] != ik_ref.CONVERGED
        assert want.status[2] == want.status[3] == ik_ref.NOT_COMPUTABLE
        assert (want.fk_status[2:4] & R.NOT_COMPUTABLE).all() and want.iterations[2] == want.iterations[3] == 0
        assert np.isnan(want.tip_pose[2, :3]).all() and np.isnan(want.error[3]).all()
        assert want.tip_pose[2, 3::4].tolist() == [0.0, 0.0, 0.0, 1.0]
    case = C.case("body13-near-B257")
    _, off = C._on_and_off_chain(case.tree, case.tip)
    want = case.want
    assert want.status[4] == want.status[5] == ik_ref.CONVERGED
    assert np.isnan(want.joints[4, off]) and want.joints[5, off] == case.seeds[5, off] > 2.0 ** 20
    assert want.fk_status[4] == 0 and want.fk_status[5] == R.OUTSIDE_LIMITS
    # columns that no chain link reads are the seed's, bit for bit
    read = {int(case.tree.joint_index[i]) for i in ik_ref.moving_links(case.tree, case.tip)}
    others = [j for j in range(case.tree.num_joints) if j not in read]
    seeds, joints = np.ascontiguousarray(case.seeds[:, others]), np.ascontiguousarray(want.joints[:, others])
    assert np.array_equal(seeds.view(np.uint64), joints.view(np.uint64))


def test_options_do_what_they_say():
    undamped = C.case("body13-undamped-B64").want
    print("undamped 4-joint chain under six weights:", np.bincount(undamped.status, minlength=4).tolist())
    assert (undamped.status == ik_ref.DEGENERATE).sum() >= 32
    none = C.case("arm-K0-B63")
    assert (none.want.iterations == 0).all() and set(none.want.status.tolist()) <= {0, 1, 3}
    assert np.array_equal(none.want.joints.view(np.uint64), none.seeds.view(np.uint64))
    short = C.case("arm-small-step-B64")
    moved = np.abs(short.want.joints - short.seeds)[short.want.fk_status == 0]
    print("max_step 0.01, 12 steps: largest change of a joint", float(moved.max()))
    assert 0.06 < moved.max() <= 12 * 0.01 * (1 + 1e-12)
    tight = C.case("arm-tight-limits-B65")
    at_limit = (np.abs(tight.want.joints) == 0.6) & (np.abs(tight.seeds) != 0.6)
    print("tight limits: entries a step pushed onto a limit", int(at_limit.sum()))
    assert at_limit.sum() > 0 and (np.abs(tight.want.joints[tight.want.fk_status == 0]) <= 0.6).all()
    position = C.case("body13-position-only-B65")
    done = position.want.status == ik_ref.CONVERGED
    assert done.sum() > 50 and (np.abs(position.want.error[done, :3]) <= 1e-6).all()
    assert (np.abs(position.want.error[done, 3:]) > 1e-3).any()
    thirds = C.case("arm-near-B63-R3")
    done = thirds.want.status == ik_ref.CONVERGED
    aim = np.repeat(thirds.targets, 3, axis=0)
    assert done.sum() > 50 and np.abs(aim[done] - thirds.want.tip_pose[done])[:, :15].max() <= 2e-6


def test_a_mimic_joint_on_the_chain_is_found():
    t = R.Tree([-1, 0, 1], [R.REVOLUTE, R.FIXED, R.PRISMATIC], [0, 0, 0], np.eye(3), np.tile(np.eye(4).reshape(16), (3, 1)), 1)
    assert ik_ref.shared_column(t, 2) == (0, 2) and ik_ref.shared_column(t, 1) is None
    body = C.tree("body")
    assert all(ik_ref.shared_column(body, tip) is None for tip in range(body.num_links))
    assert ik_ref.chain_of(body, 13) == [0, 1, 2, 9, 10, 11, 13] and ik_ref.moving_links(body, 13) == [11, 10, 9, 1]
