"""(gpu) vgt_hip_travel_cost, its device and cell-record forms and vgt_hip_trace_paths against tests/travel_ref.py.
cost, toward and num_reached are compared bit for bit; the output buffers are pre-filled with a sentinel."""
import ctypes

import numpy as np
import pytest

import travel_cases as C
import travel_ref as R
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
U = R.UNREACHED


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _run(ctx, field, weights, flags=0, sources=(), source_costs=None, cost_limit=R.NO_LIMIT, mode=R.OCCUPANCY,
         unknown_is_filled=True, threshold=0.0):
    """vgt_hip_travel_cost through the C ABI into sentinel-filled arrays -> (cost, toward, num_reached)."""
    f = np.ascontiguousarray(field, dtype=np.float32)
    src = np.ascontiguousarray(np.asarray(sources, dtype=np.int32).reshape(-1))
    costs = None if source_costs is None else np.ascontiguousarray(np.asarray(source_costs, dtype=np.uint32))
    w = np.asarray(weights, dtype=np.uint32)
    cost = np.full(f.shape, SENTINEL, dtype=np.uint32)
    toward = np.full(f.shape, SENTINEL, dtype=np.int32)
    reached = ctypes.c_int64(-7)
    capi.check(ctx._lib.vgt_hip_travel_cost(
        ctx.handle, capi._ptr(f), *f.shape, int(mode), int(bool(unknown_is_filled)), float(threshold), capi._ptr(w),
        int(flags), capi._ptr(src), capi._ptr(costs), src.size, int(cost_limit), capi._ptr(cost), capi._ptr(toward),
        ctypes.byref(reached)))
    return cost, toward, int(reached.value)


def _check(ctx, field, weights, flags=0, sources=(), source_costs=None, cost_limit=R.NO_LIMIT, mode=R.OCCUPANCY,
           unknown_is_filled=True, threshold=0.0, what=None):
    want = C.expected(field, weights, flags, sources, source_costs, cost_limit, mode, unknown_is_filled, threshold)
    got = _run(ctx, field, weights, flags, sources, source_costs, cost_limit, mode, unknown_is_filled, threshold)
    assert got[0].dtype == np.uint32 and got[1].dtype == np.int32
    assert np.array_equal(got[0], want[0]), what
    assert np.array_equal(got[1], want[1]), what
    assert got[2] == want[2], what
    return want


@pytest.mark.parametrize("flags", [0, 1], ids=["cut", "nocut"])
@pytest.mark.parametrize("weights", C.WEIGHT_SETS, ids=lambda w: "-".join(map(str, w)))
def test_every_shape_and_weight_set(ctx, weights, flags):
    reached = 0
    for shape in C.SHAPES:
        occ = C.random_occupancy(shape, 0.3)
        n = occ.size
        sources = [0] if n < 100 else [0, n - 1, int(C.random_sources(shape, 1)[0])]
        reached += _check(ctx, occ, weights, flags, sources, what=shape)[2]
    for shape in ((9, 9, 9), (17, 10, 33), (5, 23, 65), (16, 16, 64)):
        occ = C.random_occupancy(shape, 0.45, salt=1)
        reached += _check(ctx, occ, weights, flags, [0, occ.size - 1], what=shape)[2]
    assert reached > 1000


@pytest.mark.parametrize("unknown_is_filled", [False, True])
def test_edge_values_in_both_modes(ctx, unknown_is_filled):
    for shape in ((9, 9, 9), (5, 23, 65)):
        field = C.edge_values(shape)
        sources = C.random_sources(shape, 6)
        want = _check(ctx, field, (10, 14, 17), 0, sources, unknown_is_filled=unknown_is_filled)
        assert 0 < want[2] < field.size
        # thresholds equal to stored values (0.5, 0.25), beside them, and infinite
        for threshold in (0.5, 0.25, float(np.nextafter(np.float32(0.5), np.float32(0))), float("inf"), float("-inf")):
            _check(ctx, field, (10, 14, 17), 1, sources, mode=R.SDF_ABOVE, unknown_is_filled=unknown_is_filled,
                   threshold=threshold, what=threshold)


def test_serpentine_reactivates_tiles(ctx):
    occ = C.serpentine()
    want = _check(ctx, occ, (1, 0, 0), 0, [0])
    assert want[2] == 324 and int(want[0].reshape(-1)[-1]) == 323
    _check(ctx, occ, (10, 14, 17), 0, [0])
    _check(ctx, occ, (10, 14, 17), 1, [0])


def test_spiral(ctx):
    occ = C.spiral()
    want = _check(ctx, occ, (1, 0, 0), 0, [0])
    assert want[2] == int((occ == 0).sum()) and int(want[0][want[0] != U].max()) == want[2] - 1
    _check(ctx, occ, (10, 14, 17), 1, [0])


def test_nothing_to_reach(ctx):
    shape = (9, 17, 20)
    free = np.zeros(shape, np.float32)
    blocked = np.ones(shape, np.float32)
    # all cells blocked; no sources; only sources that contribute nothing (blocked, out of range, above the limit)
    mixed = C.random_occupancy(shape, 0.3)
    mixed.flat[7] = 0.0   # free, but its source starts above the limit
    mixed.flat[11] = 1.0  # blocked
    for field, sources, costs, limit in ((blocked, [0, 5], None, R.NO_LIMIT), (free, [], None, R.NO_LIMIT),
                                         (mixed, [-1, free.size, -2 ** 31, 2 ** 31 - 1, 7, 11], [0, 0, 0, 0, 9, 0], 8)):
        cost, toward, reached = _run(ctx, field, (10, 14, 17), 0, sources, costs, limit)
        assert (cost == U).all() and (toward == -1).all() and reached == 0


def test_sources(ctx):
    shape = (17, 10, 33)
    occ = C.random_occupancy(shape, 0.3)
    n = occ.size
    # duplicated sources take the least initial cost
    want = _check(ctx, occ, (10, 14, 17), 0, [0, 0, 0, n - 1, n - 1], [40, 7, 90, 3, 3])
    assert want[0].reshape(-1)[0] == 7 and want[1].reshape(-1)[0] == 0 and want[1].reshape(-1)[-1] == n - 1
    # a source dominated by another one is no root
    free = np.zeros((1, 1, 40), np.float32)
    want = _check(ctx, free, (2, 0, 0), 0, [3, 5], [0, 9])
    assert want[0][0, 0, 5] == 4 and want[1][0, 0, 5] == 4 and want[1][0, 0, 3] == 3
    want = _check(ctx, free, (2, 0, 0), 0, [3, 5], [0, 4])       # a tie: init == cost, so it is a root
    assert want[1][0, 0, 5] == 5
    # sources in different components
    walls = np.zeros(shape, np.float32)
    walls[8] = 1.0
    walls[:, :, 16] = 1.0
    want = _check(ctx, walls, (10, 14, 17), 1, [0, n - 1], [0, 1000])
    assert 0 < want[2] < int((walls == 0).sum())


def test_sources_on_tile_faces_in_corridors(ctx):
    """A corridor one cell wide: the only cell of a tile's face is the source itself, which no run of the tile lowers,
    so the neighbouring tile has to learn of it from the seed."""
    tx, ty, tz = C.TILE
    for axis, extent in ((0, tx), (1, ty), (2, tz)):
        shape = [1, 1, 1]
        shape[axis] = 2 * extent + 5
        free = np.zeros(shape, np.float32)
        for source in (extent - 1, extent, 2 * extent - 1, 2 * extent, 0, shape[axis] - 1):
            want = _check(ctx, free, (1, 0, 0), 0, [source], what=(axis, source))
            assert want[2] == free.size
    # a plate one cell thick, diagonal moves only across a tile corner: blocked everywhere but on the diagonal
    occ = np.ones((2 * tx + 3, 2 * ty + 3, 1), np.float32)
    for i in range(min(occ.shape[:2])):
        occ[i, i, 0] = 0.0
    for source in ((tx - 1) * occ.shape[1] + (ty - 1), tx * occ.shape[1] + ty):
        want = _check(ctx, occ, (10, 14, 17), 0, [source], what=source)
        assert want[2] == min(occ.shape[:2])


@pytest.mark.parametrize("limit", [0, 25, 60])
def test_cost_limit_cuts_fronts_mid_tile(ctx, limit):
    for shape in ((9, 9, 9), (17, 10, 33)):
        occ = C.random_occupancy(shape, 0.3)
        for weights in ((1, 0, 0), (10, 14, 17), (5, 0, 7)):
            want = _check(ctx, occ, weights, 0, [0, occ.size // 2], [0, 3], limit, what=(shape, weights))
            assert want[0][want[0] != U].max(initial=0) <= limit


def test_limit_equal_to_a_cells_exact_cost(ctx):
    occ = C.random_occupancy((17, 10, 33), 0.3)
    full = C.expected(occ, (10, 14, 17), 0, [0])[0]
    value = int(np.sort(full[full != U])[full.size // 4])
    want = _check(ctx, occ, (10, 14, 17), 0, [0], cost_limit=value)
    assert (want[0] == value).any() and np.array_equal(want[0] != U, full <= value)
    _check(ctx, occ, (10, 14, 17), 0, [0], cost_limit=value - 1)


def test_largest_weights_and_initial_costs_do_not_wrap(ctx):
    free = np.zeros((3, 3, 40), np.float32)
    top = R.NO_LIMIT - 65535
    want = _check(ctx, free, (65535, 65535, 65535), 0, [0, 50], [top, top - 3 * 65535])
    assert want[0].reshape(-1)[0] == top and (want[0] == R.NO_LIMIT).any() and (want[0] == U).any()
    _check(ctx, free, (65535, 0, 65534), 1, [5], [R.NO_LIMIT])


def test_device_form_with_an_exact_workspace(ctx, torch):
    shape = (17, 10, 33)
    occ = C.random_occupancy(shape, 0.3)
    sources, costs = np.array([0, occ.size - 1], np.int32), np.array([5, 0], np.uint32)
    want = C.expected(occ, (10, 14, 17), 1, sources, costs, 400)
    need = capi.travel_cost_workspace_bytes(shape)
    guard = 64
    field = torch.from_numpy(occ).cuda()
    src, cst = torch.from_numpy(sources).cuda(), torch.from_numpy(costs.view(np.int32)).cuda()
    cost = torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda")
    toward = torch.full(shape, SENTINEL, dtype=torch.int32, device="cuda")
    workspace = torch.full((need + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    reached = ctx.travel_cost_dev(field.data_ptr(), shape, src.data_ptr(), 2, cost.data_ptr(), workspace.data_ptr(), need,
                                  toward_ptr=toward.data_ptr(), source_costs_ptr=cst.data_ptr(), no_corner_cutting=True,
                                  cost_limit=400)
    assert reached == want[2]
    assert np.array_equal(cost.cpu().numpy().view(np.uint32), want[0])
    assert np.array_equal(toward.cpu().numpy(), want[1])
    assert (workspace[need:].cpu().numpy() == 0x5A).all()          # nothing behind the stated size is touched
    head = workspace[:32].cpu().numpy()
    assert int(head[16:24].view(np.uint64)[0]) == want[2] and int(head[8:12].view(np.uint32)[0]) >= 1
    # cost alone: no toward, no count
    cost.fill_(SENTINEL)
    ctx.travel_cost_dev(field.data_ptr(), shape, src.data_ptr(), 2, cost.data_ptr(), workspace.data_ptr(), need,
                        source_costs_ptr=cst.data_ptr(), no_corner_cutting=True, cost_limit=400)
    assert np.array_equal(cost.cpu().numpy().view(np.uint32), want[0])
    # one byte short: refused, nothing written
    cost.fill_(SENTINEL)
    with pytest.raises(ValueError, match="workspace"):
        ctx.travel_cost_dev(field.data_ptr(), shape, src.data_ptr(), 2, cost.data_ptr(), workspace.data_ptr(), need - 1)
    assert (cost.cpu().numpy().view(np.uint32) == SENTINEL).all()


class _DeviceRun:
    """The device form on buffers that stay: sentinel-filled outputs, a workspace of exactly the stated size."""

    def __init__(self, ctx, torch, field, weights, flags, sources, source_costs=None):
        self.ctx, self.shape = ctx, field.shape
        self.weights, self.flags = weights, flags
        self.need = capi.travel_cost_workspace_bytes(self.shape)
        self.field = torch.from_numpy(np.ascontiguousarray(field, dtype=np.float32)).cuda()
        self.sources = torch.from_numpy(np.asarray(sources, dtype=np.int32).reshape(-1)).cuda()
        costs = None if source_costs is None else np.asarray(source_costs, dtype=np.uint32).view(np.int32)
        self.costs = None if costs is None else torch.from_numpy(costs).cuda()
        self.cost = torch.empty(self.shape, dtype=torch.int32, device="cuda")
        self.toward = torch.empty(self.shape, dtype=torch.int32, device="cuda")
        self.workspace = torch.empty((self.need,), dtype=torch.uint8, device="cuda")

    def __call__(self):
        """-> (cost, toward, num_reached, the `rounds` word of the workspace's header)"""
        import torch
        self.cost.fill_(SENTINEL)
        self.toward.fill_(SENTINEL)
        self.workspace.fill_(0x5A)
        torch.cuda.synchronize()
        reached = self.ctx.travel_cost_dev(
            self.field.data_ptr(), self.shape, self.sources.data_ptr(), self.sources.numel(), self.cost.data_ptr(),
            self.workspace.data_ptr(), self.need, toward_ptr=self.toward.data_ptr(),
            source_costs_ptr=None if self.costs is None else self.costs.data_ptr(), weights=self.weights,
            no_corner_cutting=bool(self.flags & R.NO_CORNER_CUTTING))
        head = self.workspace[:32].cpu().numpy()
        assert int(head[16:24].view(np.uint64)[0]) == reached
        return (self.cost.cpu().numpy().view(np.uint32), self.toward.cpu().numpy(), reached,
                int(head[8:12].view(np.uint32)[0]))


@pytest.mark.parametrize("n", [16, 32])
def test_corridor_that_crosses_tile_faces_hundreds_of_times(ctx, torch, n):
    """C.zigzag_chain(n): one corridor that changes tile 31 times per face, so a tile is flagged by ONE neighbour 31
    times.  The rounds model (R.tile_rounds; tests/test_travel_ref.py) needs 467 rounds for n = 16 and 963 for n = 32,
    more than the tiles * 27 + 2 = 434 and 866 the host loop allowed at first, and a halo read that sees a value of the
    same launch can save a round only where two tiles are active at once: 14 rounds at n = 16, about 30 at n = 32."""
    occ = C.zigzag_chain(n)
    tiles = n
    cells = int((occ == 0).sum())
    # host form
    want = _check(ctx, occ, (1, 0, 0), 0, [0])
    assert want[2] == cells and int(want[0].reshape(-1)[C.zigzag_end(n)]) == cells - 1
    _check(ctx, occ, (10, 14, 17), R.NO_CORNER_CUTTING, [0])
    # device form: the same, in more rounds than 27 per tile and no more than the bound (vgt_hip.h, method)
    cost, toward, reached, rounds = _DeviceRun(ctx, torch, occ, (1, 0, 0), 0, [0])()
    print("zigzag_chain(%d): %d rounds on the device, tiles * 27 + 2 = %d" % (n, rounds, tiles * 27 + 2))
    assert np.array_equal(cost, want[0]) and np.array_equal(toward, want[1]) and reached == want[2]
    assert rounds > tiles * 27 + 2
    assert rounds <= occ.size + 2
    # the path from the corridor's last cell is the corridor in reverse
    end = C.zigzag_end(n)
    paths, lengths, status = ctx.trace_paths(toward, [end], cells, fill=-9)
    assert status[0] == R.TRACE_OK and lengths[0] == cells
    assert np.array_equal(want[0].reshape(-1)[paths[0]], np.arange(cells - 1, -1, -1, dtype=np.uint32))
    for g, w in zip((paths, lengths, status), R.trace_paths(want[1], [end], cells, fill=-9)):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    short = ctx.trace_paths(toward, [end], cells - 1, fill=-9)
    assert short[2][0] == R.TRACE_TRUNCATED and short[1][0] == cells - 1
    for g, w in zip(short, R.trace_paths(want[1], [end], cells - 1, fill=-9)):
        assert np.array_equal(g, w)


# The second source of test_cells_lowered_again_by_a_cheaper_front, cell (4, 32, 32): its front reaches the cells round
# it in the first rounds, at its initial cost and more, and the front from cell 0 lowers them again when it arrives.
SECOND_SOURCE = (4 * 64 + 32) * 64 + 32


@pytest.mark.parametrize("case", ["open", "blocked", "blocked-cut"])
def test_cells_lowered_again_by_a_cheaper_front(ctx, torch, case):
    """open: two fronts on a free grid, against the closed form.  blocked: 30 % blocked cells and the corner rule; there
    cell 0 reaches no other cell (the rule bars every move out of it), so one front alone re-enters tiles through the
    maze, which still lowers 9132 cells twice or more in the model.  blocked-cut: the same grid with corners cut, where
    the two sources are 466 apart; an initial cost of 300 gives each front about half of the 23 089 reached cells
    (60 would leave cell 0 one in six), and the model lowers 10 873 cells twice or more."""
    shape = (8, 64, 64)  # 32 tiles
    second_cost = 300 if case == "blocked-cut" else 60
    sources, costs = [0, SECOND_SOURCE], [0, second_cost]
    if case == "open":
        occ, weights, flags = np.zeros(shape, np.float32), (1, 0, 0), 0
    else:
        occ, weights = C.random_occupancy(shape, 0.3), (10, 14, 17)
        flags = R.NO_CORNER_CUTTING if case == "blocked" else 0
    # what the case exercises, by the rounds model: cells that a later round lowers a second time
    _, model_cost, writes, _ = R.tile_rounds(R.passable(occ), weights, flags, sources, costs, tile=C.TILE)
    again = writes >= 2
    want = C.expected(occ, weights, flags, sources, costs)
    assert np.array_equal(model_cost, want[0])
    if case == "open":
        x, y, z = np.indices(shape)
        closed_form = np.minimum(x + y + z, second_cost + abs(x - 4) + abs(y - 32) + abs(z - 32))
        assert np.array_equal(want[0], closed_form.astype(np.uint32))
        tiles = {(a // C.TILE[0], b // C.TILE[1], c // C.TILE[2]) for a, b, c in zip(*np.nonzero(again))}
        assert int(again.sum()) >= 10000 and len(tiles) >= 10
    else:
        assert int(again.sum()) > 1000
        assert want[1].reshape(-1)[SECOND_SOURCE] == SECOND_SOURCE
    if case == "blocked-cut":  # each front keeps thousands of cells: those that the other source alone leaves dearer
        from_first = C.expected(occ, weights, flags, sources[:1])[0]
        from_second = C.expected(occ, weights, flags, sources[1:], costs[1:])[0]
        assert int((from_first < from_second).sum()) > 5000 and int((from_second < from_first).sum()) > 5000
    _check(ctx, occ, weights, flags, sources, costs)
    cost, toward, reached, _ = _DeviceRun(ctx, torch, occ, weights, flags, sources, costs)()
    assert np.array_equal(cost, want[0]) and np.array_equal(toward, want[1]) and reached == want[2]


@pytest.mark.parametrize("flags", [0, 1], ids=["cut", "nocut"])
@pytest.mark.parametrize("shape", [(72, 64, 80), (33, 41, 70)], ids=["360tiles", "150tiles-partial"])
def test_hundreds_of_tiles_active_at_once(ctx, torch, shape, flags):
    """Hundreds of workgroups in one launch, so halos are read while their owners, on other XCDs too, rewrite them; the
    result is the fixed point all the same, and the same on a second call on the same buffers."""
    occ = C.random_occupancy(shape, 0.3)
    tiles = int(np.prod([-(-shape[i] // C.TILE[i]) for i in range(3)]))
    assert tiles == (360 if shape[0] == 72 else 150)
    sources, costs = [0, occ.size - 1, int(C.random_sources(shape, 1)[0])], [0, 25, 7]
    want = C.expected_large(occ, (10, 14, 17), flags, sources, costs)
    assert want[2] > occ.size // 2
    run = _DeviceRun(ctx, torch, occ, (10, 14, 17), flags, sources, costs)
    first = run()
    assert np.array_equal(first[0], want[0]) and np.array_equal(first[1], want[1]) and first[2] == want[2]
    second = run()
    assert np.array_equal(second[0], first[0]) and np.array_equal(second[1], first[1]) and second[2] == first[2]


@pytest.mark.parametrize("dtype", [capi.TAGGED_OBJECT_CELL, capi.TAGGED_OBJECT_COMPONENT_CELL], ids=["tagged8", "tagged16"])
def test_cells_form_on_a_tagged_map(ctx, dtype):
    shape = (9, 17, 20)
    rng = np.random.default_rng(11)
    rec = np.zeros(shape, dtype=dtype)
    rec["occupancy"] = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), shape, p=[0.6, 0.1, 0.3])
    rec["object_id"] = rng.integers(0, 4, shape)
    rec["occupancy"].flat[0] = 0.0
    cells = ctx.cells(rec, shape)
    sources = [0, rec.size - 1]
    for objects, unknown_is_filled in (((), True), ((), False), ((1, 3), True), ((3, 1, 3), False), ((9,), True)):
        occ = rec["occupancy"]
        filled = (occ > 0.5) | ((occ == 0.5) & unknown_is_filled)
        if objects:
            filled &= np.isin(rec["object_id"], objects)
        want = C.expected(filled.astype(np.float32), (10, 14, 17), 1, sources)
        cost, toward, reached = cells.travel_cost(sources, (10, 14, 17), objects, unknown_is_filled, no_corner_cutting=True)
        assert np.array_equal(cost, want[0]) and np.array_equal(toward, want[1]) and reached == want[2]
    cells.close()


def test_python_binding_and_two_calls_agree(ctx):
    shape = (16, 16, 64)
    occ = C.random_occupancy(shape, 0.3)
    want = C.expected(occ, (10, 14, 17), 0, [0])
    first = ctx.travel_cost(occ, [0])
    second = ctx.travel_cost(occ, [0])
    for got in (first, second):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]) and got[2] == want[2]
    cost, toward, reached = ctx.travel_cost(occ, [0], with_toward=False)
    assert toward is None and np.array_equal(cost, want[0]) and reached == want[2]


@pytest.mark.parametrize("case", ["random", "serpentine", "limited"])
def test_trace_paths_from_every_reached_cell(ctx, case):
    if case == "random":
        occ, args = C.random_occupancy((17, 10, 33), 0.3), ((10, 14, 17), 0, [0, 17 * 10 * 33 - 1])
    elif case == "serpentine":
        occ, args = C.serpentine(), ((1, 0, 0), 0, [0])
    else:
        occ, args = C.random_occupancy((9, 9, 9), 0.3), ((1, 1, 1), 1, [0, 364], [0, 2], 6)
    cost, toward, _ = C.expected(occ, *args)
    reached = np.nonzero(cost.reshape(-1) != U)[0]
    longest = int(R.trace_paths(toward, reached, occ.size)[1].max())
    starts = np.concatenate([reached, np.nonzero(cost.reshape(-1) == U)[0][:5], [-1, occ.size, -2 ** 31, 2 ** 31 - 1]])
    for max_cells in (1, longest, longest + 3, max(1, longest // 2)):
        want = R.trace_paths(toward, starts, max_cells, fill=-9)
        got = ctx.trace_paths(toward, starts, max_cells, fill=-9)
        for g, w in zip(got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), max_cells
    ok = R.trace_paths(toward, reached, longest)[2]
    assert (ok == R.TRACE_OK).all()


def test_trace_paths_malformed_toward(ctx, torch):
    toward = np.array([0, 0, 1, -1, 5, 4, 10, -7, 2, 8], np.int32)  # 4 <-> 5 cycle, 6 and 7 invalid entries, 9 -> 8 -> 2 ..
    starts = np.array([2, 3, 4, 6, 7, -1, 10, 0, 9, 5], np.int32)
    for max_cells in (1, 2, 5, 64):
        want = R.trace_paths(toward, starts, max_cells, fill=-9)
        got = ctx.trace_paths(toward, starts, max_cells, fill=-9)
        for g, w in zip(got, want):
            assert np.array_equal(g, w), max_cells
    assert want[2][2] == R.TRACE_TRUNCATED and want[1][2] == 64 and want[2][9] == R.TRACE_TRUNCATED
    # a reached cell that points at an unreached one: invalid, with the cells before it written
    broken = np.array([0, 3, 1, -1], np.int32)
    paths, lengths, status = ctx.trace_paths(broken, [2], 4, fill=-9)
    assert status[0] == R.TRACE_INVALID and lengths[0] == 2 and paths[0].tolist() == [2, 1, -9, -9]
    # the device form
    t, s = torch.from_numpy(toward).cuda(), torch.from_numpy(starts).cuda()
    paths = torch.full((len(starts), 5), -9, dtype=torch.int32, device="cuda")
    lengths = torch.full((len(starts),), -9, dtype=torch.int32, device="cuda")
    status = torch.full((len(starts),), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.trace_paths_dev(t.data_ptr(), len(toward), s.data_ptr(), len(starts), 5, paths.data_ptr(), lengths.data_ptr(),
                        status.data_ptr())
    ctx.synchronize()
    want = R.trace_paths(toward, starts, 5, fill=-9)
    assert np.array_equal(paths.cpu().numpy(), want[0]) and np.array_equal(lengths.cpu().numpy(), want[1])
    assert np.array_equal(status.cpu().numpy(), want[2])
