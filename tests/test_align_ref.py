"""(not gpu) tests/align_ref.py, the CPU restatement of vgt_hip_align_points, against its own definition: the summation
tree against an explicit loop, the estimate against the oracle, the analytic gradient against a central difference of the
restatement's own estimate, the update's orthogonality, convergence from a known offset, and the two statuses that stop a
pose where it stands.  tests/test_gpu_align.py then holds the device to this restatement bit for bit."""
import numpy as np
import pytest

import align_cases as C
import align_ref as R


def explicit_tree_sum(values):
    """The definition of include/vgt_hip.h, one scalar addition at a time."""
    v = [float(x) for x in values]
    while True:
        sums = []
        for first in range(0, len(v), 64):
            group = v[first:first + 64]
            group = group + [0.0] * (64 - len(group))
            h = 32
            while h >= 1:
                for i in range(h):
                    group[i] = group[i] + group[i + h]
                h //= 2
            sums.append(group[0])
        v = sums
        if len(v) == 1:
            return v[0]


@pytest.mark.parametrize("count", [1, 63, 64, 65, 4097])
def test_tree_sum_is_the_explicit_loop(count):
    rng = np.random.default_rng(count)
    values = rng.normal(size=count) * 10.0 ** rng.integers(-8, 8, size=count)
    got, want = R.tree_sum(values), explicit_tree_sum(values)
    assert np.float64(got).view(np.uint64) == np.float64(want).view(np.uint64)
    assert abs(got - np.sum(values)) <= 1e-12 * np.sum(np.abs(values))
    # several columns at once are the columns one by one
    columns = rng.normal(size=(count, 3))
    both = R.tree_sum(columns)
    for k in range(3):
        assert both[k].view(np.uint64) == np.float64(explicit_tree_sum(columns[:, k])).view(np.uint64)


def test_tree_sum_keeps_the_sign_of_zero_only_through_the_first_level():
    """-0.0 + +0.0 is +0.0: a group that is padded loses the sign, at any level; full groups keep it."""
    assert np.signbit(R.tree_sum(np.full(64, -0.0))) and np.signbit(R.tree_sum(np.full(4096, -0.0)))
    assert not np.signbit(R.tree_sum(np.full(63, -0.0)))
    assert not np.signbit(R.tree_sum(np.full(128, -0.0))) and not np.signbit(R.tree_sum(np.full(65, -0.0)))


def test_the_restated_estimate_is_the_oracles():
    from oracle import oracle as O
    rng = np.random.default_rng(5)
    extent = np.array(C.SHAPE) * C.RESOLUTION
    w = (rng.random((4000, 3)) * 1.2 - 0.1) * extent
    w[:200] = np.round(w[:200] / C.RESOLUTION) * C.RESOLUTION                      # on the cell lattice, faces included
    w[200:400] = (np.floor(w[200:400] / C.RESOLUTION) + 0.5) * C.RESOLUTION        # cell centres
    for xf in (None, C.projection_cases.frame_pair()[0]):
        d, _, has = R.estimate_with_gradient(C.scene(), C.RESOLUTION, w, xf)
        want, want_has = O.estimate_distance(C.scene(), C.RESOLUTION, w, xf)
        assert np.array_equal(has, want_has) and has.sum() > 1000
        assert np.array_equal(d[has].view(np.uint64), want[has].view(np.uint64))


def test_gradient_is_the_central_difference_inside_one_cell():
    """Inside one interpolation cell the interpolant is linear along each axis, so a central difference of the
    restatement's own estimate is its derivative up to rounding."""
    rng = np.random.default_rng(11)
    res = C.RESOLUTION
    # locations between the centres of cells i and i + 1, at least 0.2 cell from either, inside the grid
    base = rng.integers(1, np.array(C.SHAPE) - 2, size=(500, 3)).astype(np.float64)
    w = (base + 0.5 + 0.2 + 0.6 * rng.random((500, 3))) * res
    h = 0.05 * res
    for rotation in (None, C.projection_cases.frame_pair()[1]):
        _, g, has = R.estimate_with_gradient(C.scene(), res, w, None, None)
        assert has.all()
        numeric = np.empty_like(g)
        for axis in range(3):
            step = np.zeros(3)
            step[axis] = h
            up, _, _ = R.estimate_with_gradient(C.scene(), res, w + step)
            down, _, _ = R.estimate_with_gradient(C.scene(), res, w - step)
            numeric[:, axis] = (up - down) / (2.0 * h)
        assert np.abs(g - numeric).max() <= 1e-6
        if rotation is not None:
            _, turned, _ = R.estimate_with_gradient(C.scene(), res, w, None, rotation)
            assert np.abs(turned - g @ np.asarray(rotation).reshape(3, 3).T).max() <= 1e-12
    assert np.abs(np.linalg.norm(g, axis=1) - 1.0).mean() < 0.2                   # a distance field's gradient


def test_clamped_axis_gives_a_zero_component():
    """The two indices of an axis coincide only where the grid is one cell thick (at a face of a thicker grid the
    estimate extrapolates from the two outermost cells)."""
    res = C.RESOLUTION
    sheet = np.ascontiguousarray(C.scene()[:, :, 10:11])
    w = np.array([[0.72, 0.71, 0.2 * res], [0.43, 0.66, 0.9 * res]])
    d, g, has = R.estimate_with_gradient(sheet, res, w)
    assert has.all() and np.isfinite(d).all() and (g[:, 2] == 0.0).all() and (g[:, 0] != 0.0).all()
    edge = np.array([[0.2 * res, 0.7, 0.9]])                                       # the outer half of a face cell
    _, g, has = R.estimate_with_gradient(C.scene(), res, edge)
    assert has.all() and g[0, 0] != 0.0


def test_fifty_chained_updates_stay_orthogonal():
    rng = np.random.default_rng(3)
    pose = C.column_major(C.truth())
    for _ in range(50):
        pose = R.update(pose, rng.normal(size=6) * [0.05, 0.05, 0.05, 0.3, 0.3, 0.3], C.centre())
    rot = pose.reshape(4, 4).T[:3, :3]
    assert np.abs(rot @ rot.T - np.eye(3)).max() < 1e-12
    assert abs(np.linalg.det(rot) - 1.0) < 1e-12
    # a rotation about the pivot leaves the pivot where it is
    turned = R.update(C.column_major(np.eye(4)), [0, 0, 0, 0.2, -0.1, 0.3], C.centre())
    m = turned.reshape(4, 4).T
    assert np.abs(m[:3, :3] @ C.centre() + m[:3, 3] - C.centre()).max() < 1e-15
    # the Cayley map of omega turns by 2 atan(|omega| / 2) about omega
    angle = np.arccos((np.trace(m[:3, :3]) - 1.0) / 2.0)
    assert abs(angle - 2.0 * np.arctan(np.linalg.norm([0.2, -0.1, 0.3]) / 2.0)) < 1e-12


def test_solve_against_numpy():
    rng = np.random.default_rng(8)
    J = rng.normal(size=(40, 6))
    r = rng.normal(size=40)
    H, b = J.T @ J, J.T @ r
    sums = np.array([H[j, k] for j in range(6) for k in range(j, 6)] + list(b) + [r @ r])
    delta = R.solve(sums, 0.0)
    assert np.abs(delta + np.linalg.solve(H, b)).max() < 1e-10
    damped = R.solve(sums, 0.5)
    assert np.abs(damped + np.linalg.solve(H + 0.5 * np.diag(np.diag(H)), b)).max() < 1e-10
    flat = sums.copy()
    flat[6] = 0.0                                                                  # H_11
    flat[[1, 7, 8, 9, 10]] = 0.0                                                   # its row and column
    assert R.solve(flat, 1e-3) is None


def pose_error(pose16, truth):
    """(distance of the grid centre's images in cells, angle between the rotations in degrees)"""
    m = np.asarray(pose16).reshape(4, 4).T
    c = np.linalg.inv(truth)[:3, :3] @ C.centre() + np.linalg.inv(truth)[:3, 3]    # the centre in the sensor's frame
    moved = np.linalg.norm((m[:3, :3] @ c + m[:3, 3]) - C.centre()) / C.RESOLUTION
    relative = m[:3, :3] @ truth[:3, :3].T
    angle = np.degrees(np.arccos(np.clip((np.trace(relative) - 1.0) / 2.0, -1.0, 1.0)))
    return moved, angle


@pytest.mark.parametrize("cells,degrees", [(1.5, 3.0), (3.0, 6.0)])
def test_convergence_from_a_known_offset(cells, degrees):
    sdf, res, points, truth = C.scene(), C.RESOLUTION, C.surface_cloud(), C.truth()
    at_truth = R.evaluate(sdf, res, points, C.column_major(truth))
    assert at_truth.num_used == len(points) > 500
    target = float(np.median(at_truth.d))
    for seed in (1, 2):
        start = C.column_major(C.moved(truth, cells, degrees, seed))
        before = pose_error(start, truth)
        assert abs(before[0] - cells) < 1e-9 and abs(before[1] - degrees) < 1e-9
        got = R.align(sdf, res, points, start[None], max_iterations=30, damping=1e-3, max_residual=4.0 * res,
                      target_distance=target, translation_tolerance=1e-6 * res, rotation_tolerance=1e-8,
                      pivot=C.centre())
        after = pose_error(got.poses[0], truth)
        print("start %.1f cells %.1f deg: status %d after %d evaluations, %.2e cell %.2e deg, rms %.2e cell" % (
            cells, degrees, got.status[0], got.evaluations[0], after[0], after[1],
            np.sqrt(got.sum_squared[0] / got.num_used[0]) / res))
        assert got.status[0] == R.CONVERGED and got.evaluations[0] <= 31
        assert after[0] <= 0.05 and after[1] <= 0.05


def test_a_flat_wall_alone_is_degenerate_and_the_pose_comes_back():
    """Every gradient is (gx, 0, 0): the columns of the translations in the wall and of the rotation about its normal
    are exactly zero."""
    sdf, res = C.wall(), C.RESOLUTION
    face = C.surface_centres(True)
    face = face[(face[:, 0] > 6 * res) & (np.abs(face[:, 1] - 14 * res) < 6 * res) & (np.abs(face[:, 2] - 18 * res) < 8 * res)]
    points = C.to_cloud(face + [0.3 * res, 0.0, 0.0])
    start = C.column_major(C.moved(C.truth(), 0.2, 0.0, 4))
    ev = R.evaluate(sdf, res, points, start, target_distance=-0.5 * res, pivot=C.centre())
    assert ev.num_used == len(points) > 100
    assert (ev.gradient[:, 1] == 0.0).all() and (ev.gradient[:, 2] == 0.0).all() and (ev.gradient[:, 0] != 0.0).all()
    H = dict(zip([(j, k) for j in range(6) for k in range(j, 6)], ev.sums[:21]))
    for j in (1, 2, 3):
        assert all(value == 0.0 for (a, b), value in H.items() if j in (a, b))
    got = R.align(sdf, res, points, start[None], max_iterations=5, damping=1e-3, target_distance=-0.5 * res,
                  pivot=C.centre())
    assert got.status[0] == R.DEGENERATE and got.evaluations[0] == 1
    assert np.array_equal(got.poses[0].view(np.uint64), start.view(np.uint64))
    assert (got.last_step[0] == 0.0).all()


def test_a_cloud_sent_out_of_the_grid_has_too_few_points():
    start = C.column_major(C.matrix(np.eye(3), [5.0, 0.0, 0.0]) @ C.truth())
    for steps in (0, 5):
        got = R.align(C.scene(), C.RESOLUTION, C.surface_cloud(), start[None], max_iterations=steps)
        assert got.status[0] == R.TOO_FEW and got.num_used[0] == 0 and got.evaluations[0] == 1
        assert got.num_outside[0] == len(C.surface_cloud()) and got.num_rejected[0] == 0
        assert np.array_equal(got.poses[0].view(np.uint64), start.view(np.uint64))
    # with enough points and no step to take, the status is the iteration limit
    scored = R.align(C.scene(), C.RESOLUTION, C.surface_cloud(), C.column_major(C.truth())[None], max_iterations=0)
    assert scored.status[0] == R.ITERATION_LIMIT and scored.evaluations[0] == 1


def test_the_shared_cases_cover_what_they_promise():
    for index, (n, b, k) in enumerate(C.SHAPES):
        want = C.case(index).want
        assert want.status.shape == (b,) and want.normal_equations.shape == (b, 27)
        if n > 16:
            ordinary = slice(0, b - 1 if b > 2 else b)                              # (the last pose of a batch: one place)
            assert (want.num_outside[ordinary] >= 2).all()
            assert (want.num_used + want.num_outside + want.num_rejected == n - 3).all()   # three non-finite points
    mixed = C.case(10).want                                                        # N8197-B67-K8
    print("statuses", np.bincount(mixed.status, minlength=4).tolist(), "evaluations",
          np.bincount(mixed.evaluations).tolist())
    assert set(mixed.status.tolist()) == {R.CONVERGED, R.ITERATION_LIMIT, R.DEGENERATE, R.TOO_FEW}
    assert mixed.status[1] == R.TOO_FEW and mixed.status[-1] == R.DEGENERATE
    assert (mixed.evaluations[mixed.status == R.CONVERGED] == 3).any()              # two steps and the last evaluation
    assert (mixed.num_rejected[mixed.status == R.CONVERGED] >= 2).all()
    assert len(set(mixed.evaluations.tolist())) >= 3
