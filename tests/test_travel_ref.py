"""(not gpu) The numpy restatement of vgt_hip_travel_cost checks itself: its two forms agree, it gives the hand-derived
answers, and following `toward` strictly lowers the cost down to a root."""
import numpy as np
import pytest

import travel_cases as C
import travel_ref as R

U = R.UNREACHED


def _both(free, weights, flags, sources, source_costs=None, cost_limit=R.NO_LIMIT):
    a = R.dijkstra(free, weights, flags, sources, source_costs, cost_limit)
    b = R.bellman_ford(free, weights, flags, sources, source_costs, cost_limit)
    assert a.dtype == np.uint32 and b.dtype == np.uint32
    assert np.array_equal(a, b)
    return a


def _check_descent(free, weights, flags, cost, toward, sources, source_costs=None, cost_limit=R.NO_LIMIT):
    """Every reached cell has a toward entry; following it strictly lowers the cost and ends at a root."""
    flat_c, flat_t = cost.reshape(-1), toward.reshape(-1)
    reached = flat_c != U
    assert ((flat_t == -1) == ~reached).all()
    roots = flat_t == np.arange(flat_t.size)
    init = R._contributing(free, sources, source_costs, cost_limit)
    for r in np.nonzero(roots)[0]:
        assert init[int(r)] == int(flat_c[r])
    step = reached & ~roots
    assert (flat_c[flat_t[step]] < flat_c[step]).all()
    paths, lengths, status = R.trace_paths(toward, np.nonzero(reached)[0], flat_t.size)
    assert (status == R.TRACE_OK).all()
    ends = paths[np.arange(len(paths)), lengths - 1]
    assert roots[ends].all()


def test_corridor():
    free = np.ones((1, 1, 5), bool)
    cost = _both(free, (1, 0, 0), 0, [0])
    assert cost.reshape(-1).tolist() == [0, 1, 2, 3, 4]
    toward = R.toward(free, (1, 0, 0), 0, cost, [0])
    assert toward.reshape(-1).tolist() == [0, 0, 1, 2, 3]
    cost = _both(free, (3, 0, 0), 0, [4, 0], [1, 2])
    assert cost.reshape(-1).tolist() == [2, 5, 7, 4, 1]
    assert R.toward(free, (3, 0, 0), 0, cost, [4, 0], [1, 2]).reshape(-1).tolist() == [0, 0, 3, 4, 4]


PLATE = {  # a 3 x 3 x 1 plate, centre blocked, source in the corner (0, 0); cells in linear order, X = unreached
    ((1, 0, 0), 0): [0, 1, 2, 1, U, 3, 2, 3, 4],
    ((2, 3, 0), 0): [0, 2, 4, 2, U, 5, 4, 5, 7],
    ((10, 14, 17), 0): [0, 10, 20, 10, U, 24, 20, 24, 34],
    ((1, 1, 1), 0): [0, 1, 2, 1, U, 2, 2, 2, 3],
    ((5, 0, 7), 0): [0, 5, 10, 5, U, 15, 10, 15, 20],
    # every 2 x 2 block of the plate holds the centre: the corner rule leaves the axis moves only
    ((2, 3, 0), 1): [0, 2, 4, 2, U, 6, 4, 6, 8],
    ((10, 14, 17), 1): [0, 10, 20, 10, U, 30, 20, 30, 40],
    ((1, 1, 1), 1): [0, 1, 2, 1, U, 3, 2, 3, 4],
}


@pytest.mark.parametrize("weights,flags", sorted(PLATE))
def test_plate_with_a_blocked_centre(weights, flags):
    free = np.ones((3, 3, 1), bool)
    free[1, 1, 0] = False
    cost = _both(free, weights, flags, [0])
    assert cost.reshape(-1).tolist() == PLATE[(weights, flags)]
    toward = R.toward(free, weights, flags, cost, [0])
    assert toward[0, 0, 0] == 0 and toward[1, 1, 0] == -1
    _check_descent(free, weights, flags, cost, toward, [0])


def test_plate_toward_takes_the_first_offset_in_order():
    """{1,1,1} on the free plate from the centre: cost 1 everywhere else, and every cell points at the centre; from the
    corner, cell (1, 2) costs 2 with three cells at cost 1 beside it... the first in (dx, dy, dz) order wins."""
    free = np.ones((3, 3, 1), bool)
    cost = _both(free, (1, 1, 1), 0, [0])
    assert cost.reshape(-1).tolist() == [0, 1, 2, 1, 1, 2, 2, 2, 2]
    toward = R.toward(free, (1, 1, 1), 0, cost, [0]).reshape(-1).tolist()
    # (0,2): neighbours at cost 1 are (0,1) [d = (0,-1,0)] and (1,1) [d = (1,-1,0)]: (0,-1,0) comes first
    # (1,2): (0,1) [d = (-1,-1,0)] before (1,1) [d = (0,-1,0)];  (2,2): only (1,1);  (2,0): (1,0) [(-1,0,0)] before (1,1)
    assert toward == [0, 0, 1, 0, 0, 1, 3, 3, 4]


def test_diagonal_gap_with_and_without_the_corner_rule():
    free = np.array([[[True], [False]], [[False], [True]]])  # (0,0) and (1,1) free
    cost = _both(free, (10, 14, 17), 0, [0])
    assert cost.reshape(-1).tolist() == [0, U, U, 14]
    cost = _both(free, (10, 14, 17), R.NO_CORNER_CUTTING, [0])
    assert cost.reshape(-1).tolist() == [0, U, U, U]
    # the same in 3-D: a class-3 move through a 2 x 2 x 2 block with one blocked cell
    free = np.ones((2, 2, 2), bool)
    free[0, 1, 1] = False
    assert _both(free, (10, 14, 17), 0, [0])[1, 1, 1] == 17
    assert _both(free, (10, 14, 17), R.NO_CORNER_CUTTING, [0])[1, 1, 1] == 24


def test_serpentine():
    occ = C.serpentine()
    free = R.passable(occ)
    assert int(free.sum()) == 324
    cost = _both(free, (1, 0, 0), 0, [0])
    assert int((cost != U).sum()) == 324 and int(cost.reshape(-1)[-1]) == 323
    toward = R.toward(free, (1, 0, 0), 0, cost, [0])
    _check_descent(free, (1, 0, 0), 0, cost, toward, [0])
    paths, lengths, status = R.trace_paths(toward, [free.size - 1], 400)
    assert status[0] == R.TRACE_OK and lengths[0] == 324 and paths[0, 323] == 0


def test_spiral_is_one_corridor():
    occ = C.spiral()
    free = R.passable(occ)
    cost = _both(free, (1, 0, 0), 0, [0])
    assert int((cost != U).sum()) == int(free.sum())
    # a corridor: every length up to the longest occurs exactly once
    reached = np.sort(cost[cost != U])
    assert np.array_equal(reached, np.arange(len(reached)))
    assert len(reached) > 9 * (5 * 33 + 4)


@pytest.mark.parametrize("n,rounds", [(4, 95), (16, 467), (32, 963)])
def test_zigzag_chain_is_one_corridor_that_needs_more_rounds_than_27_per_tile(n, rounds):
    occ = C.zigzag_chain(n)
    assert occ.shape == (C.TILE[0], C.TILE[1] * n, C.TILE[2]) and occ.dtype == np.float32
    free = R.passable(occ)
    cells = int(free.sum())
    assert cells == 7 + 98 * (n - 1) + 12 * (n - 2)
    got_rounds, cost, writes, most_active = R.tile_rounds(free, (1, 0, 0), 0, [0], tile=C.TILE)
    assert cost.dtype == np.uint32 and np.array_equal(cost, R.bellman_ford(free, (1, 0, 0), 0, [0]))
    if n == 4:
        assert np.array_equal(cost, R.dijkstra(free, (1, 0, 0), 0, [0]))
    # one corridor without branches: every free cell is reached, and every length up to the longest occurs once
    reached = np.sort(cost[cost != U])
    assert np.array_equal(cost != U, free) and np.array_equal(reached, np.arange(cells))
    assert int(cost.reshape(-1)[C.zigzag_end(n)]) == cells - 1
    # it changes tile 31 times per face between two tiles
    path = np.argsort(cost.reshape(-1), kind="stable")[:cells]
    tile_of = np.unravel_index(path, occ.shape)[1] // C.TILE[1]
    assert int(np.count_nonzero(np.diff(tile_of))) == 31 * (n - 1)
    once = free.copy()
    once.flat[0] = False  # (the source is seeded, not lowered)
    assert np.array_equal(writes, once.astype(np.int64)) and most_active == 2  # every other cell is lowered once
    # the rounds of the model, and what the host loop allowed before: tiles * 27 + 2
    assert got_rounds == rounds
    assert (got_rounds > n * 27 + 2) == (n >= 16)
    assert got_rounds <= occ.size + 2


@pytest.mark.parametrize("case", ["serpentine", "spiral"])
def test_tile_rounds_reaches_the_same_field(case):
    occ = C.serpentine() if case == "serpentine" else C.spiral()
    free = R.passable(occ)
    for weights, flags in (((1, 0, 0), 0), ((10, 14, 17), 0), ((10, 14, 17), 1)):
        rounds, cost, writes, most_active = R.tile_rounds(free, weights, flags, [0], tile=C.TILE)
        assert np.array_equal(cost, C.expected(occ, weights, flags, [0])[0]), (weights, flags)
        assert rounds > 1 and most_active >= 1 and int(writes.max()) >= 1
        assert np.array_equal(writes > 0, (cost != U) & (np.arange(cost.size).reshape(cost.shape) != 0))


def test_tile_rounds_with_sources_costs_and_a_limit():
    shape = (17, 10, 33)
    occ = C.random_occupancy(shape, 0.3)
    free = R.passable(occ)
    sources, costs = [0, occ.size - 1, -4, occ.size // 2], [5, 0, 0, 900]
    for limit in (R.NO_LIMIT, 400):
        rounds, cost, writes, _ = R.tile_rounds(free, (10, 14, 17), 1, sources, costs, limit, tile=C.TILE)
        assert np.array_equal(cost, C.expected(occ, (10, 14, 17), 1, sources, costs, limit)[0])
    # another tile size gives the same field
    assert np.array_equal(R.tile_rounds(free, (10, 14, 17), 1, sources, costs, 400, tile=(4, 5, 7))[1], cost)
    # no contributing source: no round
    rounds, cost, writes, most_active = R.tile_rounds(free, (1, 0, 0), 0, [-1, occ.size])
    assert (rounds, most_active) == (0, 0) and (cost == U).all() and not writes.any()


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_graph_cost_agrees_with_bellman_ford(shape):
    occ = C.random_occupancy(shape, 0.3)
    free = R.passable(occ)
    n = occ.size
    sources, costs = [0, n - 1, int(C.random_sources(shape, 1)[0]), n - 1, -1, n], [0, 25, 7, 30, 0, 0]
    for weights, flags in (((10, 14, 17), 0), ((10, 14, 17), 1), ((1, 0, 0), 0), ((5, 0, 7), 1)):
        for limit in (R.NO_LIMIT, 60):
            got = R.graph_cost(free, weights, flags, sources, costs, limit)
            assert got.dtype == np.uint32 and got.shape == shape
            assert np.array_equal(got, R.bellman_ford(free, weights, flags, sources, costs, limit)), (weights, flags, limit)


def test_limits_and_wrap():
    free = np.ones((1, 1, 4), bool)
    top = R.NO_LIMIT - 65535
    cost = _both(free, (65535, 0, 0), 0, [0], [top])
    assert cost.reshape(-1).tolist() == [top, R.NO_LIMIT, U, U]
    cost = _both(free, (1, 0, 0), 0, [0], None, 2)
    assert cost.reshape(-1).tolist() == [0, 1, 2, U]
    assert _both(free, (1, 0, 0), 0, [0], [3], 2).reshape(-1).tolist() == [U] * 4


def test_passable_follows_the_segment_cast():
    f = np.array([np.nan, np.inf, -np.inf, 0.5, 0.25, 0.75], np.float32).reshape(1, 1, 6)
    assert R.passable(f, R.OCCUPANCY, True).reshape(-1).tolist() == [True, False, True, False, True, False]
    assert R.passable(f, R.OCCUPANCY, False).reshape(-1).tolist() == [True, False, True, True, True, False]
    assert R.passable(f, R.SDF_ABOVE, True, 0.5).reshape(-1).tolist() == [True, True, False, False, False, True]
    assert R.passable(f, R.SDF_ABOVE, True, np.inf).reshape(-1).tolist() == [True, False, False, False, False, False]


@pytest.mark.parametrize("seed", range(12))
def test_random_grids_agree_and_descend(seed):
    rng = np.random.default_rng(1000 + seed)
    shape = tuple(int(v) for v in rng.integers(1, 8, 3))
    free = rng.random(shape) >= 0.35
    n = free.size
    sources = rng.integers(-1, n + 1, 3)
    costs = rng.integers(0, 30, 3)
    for weights in C.WEIGHT_SETS:
        for flags in (0, 1):
            for limit in (R.NO_LIMIT, 25, 0):
                cost = _both(free, weights, flags, sources, costs, limit)
                toward = R.toward(free, weights, flags, cost, sources, costs, limit)
                _check_descent(free, weights, flags, cost, toward, sources, costs, limit)


@pytest.mark.parametrize("shape", [(9, 9, 9), (7, 9, 15), (5, 23, 65)])
def test_shared_cases_agree(shape):
    occ = C.random_occupancy(shape, 0.3)
    free = R.passable(occ)
    for weights, flags in (((10, 14, 17), 0), ((5, 0, 7), 1)):
        want = C.expected(occ, weights, flags, [0])[0]
        assert np.array_equal(R.dijkstra(free, weights, flags, [0]), want)


def test_trace_statuses():
    toward = np.array([0, 0, 1, -1, 5, 4, 9, -7], np.int32)  # 4 <-> 5 is a cycle, 6 points outside, 7 below -1
    paths, lengths, status = R.trace_paths(toward, [2, 3, 4, 6, 7, -1, 8, 0, 2], 2, fill=-9)
    assert status.tolist() == [R.TRACE_TRUNCATED, R.TRACE_UNREACHED, R.TRACE_TRUNCATED, R.TRACE_INVALID, R.TRACE_INVALID,
                               R.TRACE_INVALID, R.TRACE_INVALID, R.TRACE_OK, R.TRACE_TRUNCATED]
    assert lengths.tolist() == [2, 0, 2, 0, 0, 0, 0, 1, 2]
    assert paths[0].tolist() == [2, 1] and paths[2].tolist() == [4, 5] and paths[7].tolist() == [0, -9]
    paths, lengths, status = R.trace_paths(toward, [2], 3)
    assert status[0] == R.TRACE_OK and paths[0].tolist() == [2, 1, 0]
