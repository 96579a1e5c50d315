"""(not gpu) The CPU oracle's SDF consumers against tests/consumer_ref.py, the numpy restatement written from the
reference header: values bit for bit, has_value, NaN placement and the window-too-large flag equal, on every case of
tests/consumer_cases.py (the cases tests/test_gpu_consumers.py runs on the device).  Then what the restatement itself
must satisfy by definition, and that the case builders reach what they are there for."""
import numpy as np
import pytest

import consumer_cases as C
import consumer_ref as R
from oracle import oracle as O


def same_doubles(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(nan_a, nan_b) and \
        np.array_equal(a[~nan_a].view(np.uint64), b[~nan_b].view(np.uint64))


FIELD_IDS = ["%s-%s" % (kind, "x".join(map(str, shape))) for kind, shape in C.FIELD_AND_SHAPE]


@pytest.mark.parametrize("kind,shape", C.FIELD_AND_SHAPE, ids=FIELD_IDS)
def test_coarse_gradient_matches_oracle(kind, shape):
    for case in C.field_cases([kind], [shape]):
        for edges in (False, True):
            for frame in ("grid", "quarter_turn", "rigid"):
                rot = C.rotation(frame)
                want, whas = O.coarse_gradient(case.field, case.resolution, edges, rot)
                got, has = R.coarse_gradient(case.field, case.resolution, edges, rot)
                assert np.array_equal(has, whas), (case.name, edges, frame)
                assert same_doubles(got, want), (case.name, edges, frame)
                assert np.isnan(got[~has]).all()


@pytest.mark.parametrize("kind,shape", C.FIELD_AND_SHAPE, ids=FIELD_IDS)
def test_estimate_matches_oracle(kind, shape):
    for case in C.query_cases(kind, shape):
        want, whas = O.estimate_distance(case.field, case.resolution, case.queries, case.grid_from_world)
        got, has = R.estimate_distance(case.field, case.resolution, case.queries, case.grid_from_world)
        assert np.array_equal(has, whas), case.name
        assert same_doubles(got, want), case.name
        assert np.isnan(got[~has]).all(), case.name
        assert has.any() and not has.all(), case.name            # points in the grid and points outside it


def test_queries_sit_where_they_are_meant_to():
    """In the grid frame the centre queries have offset 0.0 on every axis, boundary queries k * res land in cell k or, at
    a resolution that is no power of two, in cell k - 1; both happen."""
    lands_below = 0
    for res in C.RESOLUTIONS:
        shape = (33, 3, 64)
        q = C.grid_queries(shape, res)
        cells = int(np.prod(shape))
        centres = q[:cells]
        idx = np.floor(centres * (1.0 / res))
        assert np.array_equal(idx.reshape(shape + (3,)), np.indices(shape).transpose(1, 2, 3, 0))
        assert np.all(centres - (idx + 0.5) * res == 0.0)
        k = np.arange(65)
        lands_below += int(np.count_nonzero(np.floor((k * res) * (1.0 / res)) == k - 1))
    assert lands_below > 0
    # the specials are there: -0.0, the smallest negative double, NaN and both infinities
    q = C.grid_queries((2, 2, 2), 0.1)
    assert np.any(np.signbit(q) & (q == 0.0)) and np.any(q == -5e-324) and np.isnan(q).any() and np.isinf(q).any()


FINE = C.fine_cases()


@pytest.mark.parametrize("case", FINE, ids=[c.name for c in FINE])
def test_fine_gradient_matches_oracle(case):
    want, whas, wflag = O.fine_gradient(case.field, case.resolution, case.queries, case.window, case.grid_from_world)
    got, has, flag = R.fine_gradient(case.field, case.resolution, case.queries, case.window, case.grid_from_world)
    assert flag == wflag == case.raises, case.name
    assert np.array_equal(has, whas) and same_doubles(got, want), case.name
    assert np.isnan(got[~has]).all()


def test_fine_gradient_sets_take_their_branches():
    """Branches of ComputeAxisFineGradient taken by the sets, counted with the restatement (queries per set; the set of
    (branch, axis) takes that branch on that axis and the two-sided one on the two others):

        frame         minus_only x/y/z   plus_only x/y/z   both (all axes)
        grid          589 / 547 / 523    533 / 543 / 543   2223
        quarter_turn  543 / 589 / 523    547 / 533 / 543   2223
        rigid         144 / 197 / 292    131 / 200 / 290   2731

    (axes of the query's frame).  negative_window: all 6000 candidates but those that throw, every branch occurs (the
    window is fabs'd; with its sign kept the one-sided queries would swap sides).  thin_axis: 64 queries in the grid,
    every one without a neighbour on z -> the call raises.  good_only: 40 queries, each one-sided on some axis (grid
    frame: 20 plus-only and 20 minus-only on z, x and y two-sided).  one_thrower: the same 40 and one query in the
    middle band -> raises.  outside_only: no query in the grid, no value, no error."""
    counts = {}
    for case in FINE:
        branches = R.fine_gradient_branches(case.field, case.resolution, case.queries, case.window, case.grid_from_world)
        name = case.name.split("-", 1)[1]
        if case.branch is not None:
            assert len(case.queries) > 0, case.name
            others = [a for a in range(3) if a != case.axis]
            assert (branches[:, case.axis] == case.branch).all(), case.name
            assert (branches[:, others] == R.BRANCH_BOTH).all(), case.name
            counts[case.name] = len(case.queries)
        elif name == "negative_window":
            assert set(np.unique(branches)) == {R.BRANCH_BOTH, R.BRANCH_MINUS_ONLY, R.BRANCH_PLUS_ONLY}
        elif name == "thin_axis":
            assert len(case.queries) == 64 and (branches[:, 2] == R.BRANCH_NONE).all()
        elif name == "good_only":
            assert len(case.queries) == 40 and not (branches == R.BRANCH_NONE).any() and (branches >= 0).all()
            assert (branches != R.BRANCH_BOTH).any(axis=1).all()
            if case.grid_from_world is None:
                assert np.bincount(branches[:, 2], minlength=4).tolist() == [0, 20, 20, 0]
                assert (branches[:, :2] == R.BRANCH_BOTH).all()
        elif name == "one_thrower":
            assert np.count_nonzero((branches == R.BRANCH_NONE).any(axis=1)) == 1
        else:
            assert name == "outside_only" and (branches == -1).all()
    print(counts)
    assert len(counts) == 27
    # a rotated frame steps the window along the world's axes: stepping along the grid's instead changes the values
    case = next(c for c in FINE if c.name == "rigid-both-axis0")
    got, _, _ = R.fine_gradient(case.field, case.resolution, case.queries, case.window, case.grid_from_world)
    in_grid = np.stack(R.to_grid_frame(case.queries, case.grid_from_world), axis=1)
    other, _, _ = R.fine_gradient(case.field, case.resolution, in_grid, case.window, None)
    assert not np.allclose(got, other)


EXTREMA = C.extrema_cases()


@pytest.mark.parametrize("case", EXTREMA, ids=[c.name for c in EXTREMA])
def test_local_extrema_map_matches_oracle(case):
    want = O.local_extrema_map(case.field, case.resolution, case.rotation)
    got = R.local_extrema_map(case.field, case.resolution, case.rotation)
    assert not np.isnan(got).any() and not (got == -np.inf).any()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), case.name


def _centres(shape, res):
    return np.stack(np.meshgrid(*[(np.arange(n, dtype=np.float64) + 0.5) * res for n in shape], indexing="ij"), axis=-1)


# ---- what the restatement must satisfy by definition ----
@pytest.mark.parametrize("shape", [(9, 8, 10), (1, 6, 5), (2, 2, 2), (1, 1, 1)])
def test_estimate_at_centres_is_the_corrected_centre_value(shape):
    """At a cell centre both interpolation weights are exactly 0 and 1, so the estimate is the cell's own value moved
    half a cell towards zero (+0.0 and -0.0 count as outside: down)."""
    res = 0.125
    for kind in ("normal", "signed_zero"):
        f = C.field(kind, shape)
        got, has = R.estimate_distance(f, res, _centres(shape, res).reshape(-1, 3))
        nominal = f.astype(np.float64).reshape(-1)
        want = np.where(nominal >= 0.0, nominal - res * 0.5, nominal + res * 0.5)
        assert has.all() and np.array_equal(got, want)


def test_affine_fields_are_reproduced():
    """f = a x + b y + c z + d with three distinct coefficients, positive all over the grid, stored as float32: the
    estimate is f - res / 2 everywhere in the grid (the border half cells extrapolate), and the fine gradient under a
    rotated frame is the coefficient vector turned into the world.

    Bound: every stored value is off by at most max|f| * 2^-24 (float32 rounding).  The estimate weighs eight of them
    with weights whose absolute values sum to at most 2 per axis (t in [-1/2, 3/2]), 8 in all; the fine gradient divides
    the difference of two estimates by at least one window.  The double arithmetic adds a few 2^-53 relative, covered
    by one more 2^-24 term.  So: estimate 9 * max|f| * 2^-24, gradient 18 * max|f| * 2^-24 / window.
    Measured (restatement and oracle alike): estimate 6.7e-07 of a bound of 4.0e-06; gradient 9.1e-06 (quarter turn)
    and 7.2e-06 (rigid) of a bound of 2.7e-04."""
    shape, res, window = (9, 8, 10), 0.1, 0.03
    coefficients = np.array([0.7, -1.3, 2.1])
    centres = _centres(shape, res)
    f = (centres @ coefficients + 5.0).astype(np.float32)
    assert f.min() > 0.0
    peak = float(np.abs(f).max())
    rng = np.random.default_rng(2)
    q_grid = rng.random((4000, 3)) * np.array(shape) * res
    for estimate, fine in ((R.estimate_distance, R.fine_gradient), (O.estimate_distance, O.fine_gradient)):
        got, has = estimate(f, res, q_grid)
        deviation = np.abs(got - (q_grid @ coefficients + 5.0 - res * 0.5)).max()
        print("estimate deviation", deviation, "bound", 9 * peak * 2.0 ** -24)
        assert has.all() and deviation <= 9 * peak * 2.0 ** -24
        for frame in C.ROTATED_FRAMES:
            q = C.to_world(q_grid, frame)
            # (near an edge of the grid a step along an oblique world axis leaves on both sides: the reference throws)
            q = q[~(R.fine_gradient_branches(f, res, q, window, C.grid_from_world(frame)) == R.BRANCH_NONE).any(axis=1)]
            grad, ghas, flag = fine(f, res, q, window, C.grid_from_world(frame))
            want = C.rotation(frame) @ coefficients
            deviation = np.abs(grad[ghas] - want).max()
            print(frame, "gradient deviation", deviation, "bound", 18 * peak * 2.0 ** -24 / window)
            assert not flag and ghas.sum() > 3900 and deviation <= 18 * peak * 2.0 ** -24 / window


@pytest.mark.parametrize("shape", C.SHAPES)
def test_constant_and_infinite_fields_are_their_own_extrema(shape):
    """A constant field is flat everywhere.  In a field of one infinity every difference is NaN (or 0.0 along an axis of
    one cell): not flat and no move, so the walk is back at once.  Either way: every cell's own centre."""
    res = 0.1
    for value in (0.0, -2.5, np.inf, -np.inf):
        got = R.local_extrema_map(np.full(shape, value, dtype=np.float32), res, C.rotation("rigid"))
        assert np.array_equal(got, _centres(shape, res))


# ---- the extrema fields reach what they are there for ----
def test_threshold_fields_straddle_the_step():
    step = C.THRESHOLD_RES * R.STEP_FACTOR
    for name, f, target, axis, sign, moves in C.threshold_fields():
        grad, _ = R.coarse_gradient(f, C.THRESHOLD_RES, True)
        g = grad[target][axis] * sign
        other = np.delete(grad[target], axis)
        assert (g > step) == moves and np.all(other == 0.0), name
        # the nearest representable gradient on that side: one float32 step of the neighbour crosses the threshold
        assert abs(g - step) < step * 2.0 ** -22, name
        flat, nxt = R.successors(f, C.THRESHOLD_RES)
        cell = (target[0] * 5 + target[1]) * 5 + target[2]
        stride = (25, 5, 1)[axis]
        successor = cell + int(sign) * stride if moves else cell
        if moves and sign < 0 and target[axis] == 0:
            successor = -1                                       # down from the lower face: off the grid
        assert flat[cell] == (not moves) and nxt[cell] == successor, name


def test_ramps_and_ring():
    n = C.RAMP_CELLS
    flat, nxt = R.successors(C.ramp("flat"), C.RAMP_RES)
    assert flat.tolist() == [False] * (n - 1) + [True] and nxt[:-1].tolist() == list(range(1, n))
    got = R.local_extrema_map(C.ramp("flat"), C.RAMP_RES)
    assert np.all(got[0, 0, :, 2] == (n - 1 + 0.5) * C.RAMP_RES)
    flat, nxt = R.successors(C.ramp("two_cycle"), C.RAMP_RES)
    assert not flat.any() and nxt.tolist() == list(range(1, n)) + [n - 2]
    got = R.local_extrema_map(C.ramp("two_cycle"), C.RAMP_RES)
    assert np.all(got[0, 0, :, 2] == (n - 2 + 0.5) * C.RAMP_RES)          # the chain from cell 0 enters at 4094
    flat, nxt = R.successors(C.ramp("off_grid"), C.RAMP_RES)
    assert not flat.any() and nxt.tolist() == list(range(1, n)) + [-1]
    assert np.all(R.local_extrema_map(C.ramp("off_grid"), C.RAMP_RES) == np.inf)
    # the ring: a cycle of four cells; the smallest cell of its basin is cell 2, on the cycle
    flat, nxt = R.successors(C.ring_field(), C.RING_RES)
    ring = C.RING_CELLS
    assert len(ring) > 2 and [int(nxt[c]) for c in ring] == ring[1:] + ring[:1] and not flat[ring].any()
    basin = []
    for start in range(36):
        cell, seen = start, set()
        while cell >= 0 and not flat[cell] and cell not in seen:
            seen.add(cell)
            cell = int(nxt[cell])
        if cell in ring:
            basin.append(start)
    assert min(basin) == min(ring) == 2 and len(basin) > len(ring)
    got = R.local_extrema_map(C.ring_field(), C.RING_RES).reshape(36, 3)
    assert np.all(got[basin] == [0.5, 0.5, 2.5])


def test_signed_zero_and_non_finite_cells_decide_moves():
    """-0.0 climbs (it is not < 0) where -1e-45 descends, with a gradient that is not flat; a NaN gradient is neither
    flat nor a move."""
    f = C.field("signed_zero", (9, 8, 10))
    flat, nxt = R.successors(f, 0.125)
    cells = np.arange(f.size)
    values = f.reshape(-1)
    moving = ~flat & (nxt != cells)
    assert np.count_nonzero(moving & (values == 0.0) & np.signbit(values)) > 10
    assert np.count_nonzero(moving & (values == -C.TINY)) > 10 and np.count_nonzero(moving & (values == C.TINY)) > 10
    f = C.field("non_finite", (9, 8, 10))
    flat, nxt = R.successors(f, 0.125)
    grad, _ = R.coarse_gradient(f, 0.125, True)
    nan_gradient = np.isnan(grad).any(axis=-1).reshape(-1)
    assert nan_gradient.sum() >= 6 and not flat[nan_gradient].any()
    assert np.isinf(grad).any()
