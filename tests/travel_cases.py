"""Inputs for the travel-cost tests, shared by the restatement's own tests and the GPU tests, and the cached expected
results (computed once per case, never modified: the arrays are read-only)."""
import functools

import numpy as np

import travel_ref as R

# The tile a workgroup relaxes; the shapes below sit on both sides of one and of two tile extents.
TILE = (8, 8, 16)

WEIGHT_SETS = [(1, 0, 0), (2, 3, 0), (10, 14, 17), (1, 1, 1), (5, 0, 7)]
SHAPES = [(1, 1, 1), (1, 1, 70), (1, 70, 1), (70, 1, 1), (8, 8, 8), (9, 9, 9), (17, 10, 33), (5, 23, 65), (16, 16, 64),
          # one cell less / more than one and than two tile extents, per axis
          (7, 9, 15), (9, 7, 17), (15, 17, 31), (17, 15, 33)]


def _seed(shape, salt):
    return (shape[0] * 1000003 + shape[1] * 1009 + shape[2]) * 16 + salt


def random_occupancy(shape, blocked=0.3, salt=0):
    """Float occupancy, `blocked` of the cells 1.0 and the rest 0.0; cell 0 and the last cell are free."""
    rng = np.random.default_rng(_seed(shape, salt))
    occ = (rng.random(shape) < blocked).astype(np.float32)
    occ.flat[0] = 0.0
    occ.flat[-1] = 0.0
    return occ


def random_sources(shape, count, salt=0):
    rng = np.random.default_rng(_seed(shape, 7 + salt))
    return rng.integers(0, int(np.prod(shape)), count).astype(np.int32)


def edge_values(shape, salt=0):
    """A field with NaN, +-inf, exactly 0.5 and ordinary values on both sides of it."""
    rng = np.random.default_rng(_seed(shape, 3 + salt))
    values = np.array([np.nan, np.inf, -np.inf, 0.5, 0.0, 1.0, 0.25, 0.75, -0.5, np.nextafter(np.float32(0.5), np.float32(1)),
                       np.nextafter(np.float32(0.5), np.float32(0))], dtype=np.float32)
    weights = np.array([2, 1, 1, 3, 6, 2, 3, 2, 2, 1, 1], dtype=np.float64)
    return rng.choice(values, shape, p=weights / weights.sum()).astype(np.float32)


def serpentine(ny=25, nz=24):
    """The 1 x ny x nz comb: blocked rows at odd y with one gap, alternating between z = nz - 1 and z = 0; the source is
    cell 0.  One corridor that crosses the tiles dozens of times."""
    occ = np.zeros((1, ny, nz), dtype=np.float32)
    for y in range(1, ny, 2):
        occ[0, y, :] = 1.0
        occ[0, y, nz - 1 if (y // 2) % 2 == 0 else 0] = 0.0
    return occ


def spiral(shape=(17, 10, 33)):
    """A 3-D corridor of the same kind: in every even x slab a serpentine in (y, z), the slabs at odd x blocked except
    for one cell, alternately at the far end and at the start of the slab's corridor."""
    nx, ny, nz = shape
    occ = np.ones(shape, dtype=np.float32)
    flip = False
    # the slab's corridor runs 0 -> nz - 1 in row 0, back in row 2, ...: from (0, 0) to the end of the last even row
    last_row = ny - 1 if (ny - 1) % 2 == 0 else ny - 2
    far = (last_row, (nz - 1) if (last_row // 2) % 2 == 0 else 0)
    for x in range(0, nx, 2):
        occ[x] = serpentine(ny, nz)[0]
        occ[x, last_row + 1:, :] = 1.0  # (no spur behind the corridor's end)
        if x + 1 < nx:
            y, z = (0, 0) if flip else far
            occ[x + 1, y, z] = 0.0
            flip = not flip
    return occ


def zigzag_chain(n_tiles):
    """8 x 8 * n_tiles x 16, a chain of tiles along Y, blocked but for ONE corridor without branches that crosses every
    face between two tiles 31 times: the rows x = 0, 2, 4, 6 on both sides of the face run along Z with every fourth
    cell blocked, on the two sides in turn, so that the corridor changes side every second cell.  A tile therefore hears
    of a lowered face cell 31 times per face, not once; the source is cell 0 and the last cell is zigzag_end()."""
    tx, ty, tz = TILE
    occ = np.ones((tx, ty * n_tiles, tz), dtype=np.float32)
    z = np.arange(tz)
    occ[0, 0:ty - 1, 0] = 0.0                                 # lead-in to the first face
    for j in range(n_tiles - 1):
        a, b = ty * j + ty - 1, ty * j + ty                   # the last row of tile j, the first of tile j + 1
        for x in (0, 2, 4, 6):
            occ[x, a, z[z % 4 != 1]] = 0.0
            occ[x, b, z[z % 4 != 3]] = 0.0
        occ[1, a, tz - 1] = occ[3, a, 0] = occ[5, a, tz - 1] = 0.0   # from one row to the next, on side a
        occ[6, a, 0] = 1.0                                    # the last row ends on side b, after 7 crossings
        if j < n_tiles - 2:                                   # on to the next face
            occ[6, b + 1:b + 4, 0] = 0.0
            occ[0:7, b + 3, 0] = 0.0
            occ[0, b + 3:b + 7, 0] = 0.0
    return occ


def zigzag_end(n_tiles):
    """Linear index of the last cell of zigzag_chain(n_tiles)'s corridor: (6, first row of the last tile, 0)."""
    tx, ty, tz = TILE
    return (6 * ty * n_tiles + ty * (n_tiles - 1)) * tz


@functools.lru_cache(maxsize=None)
def _expected(key):
    field, weights, flags, sources, source_costs, cost_limit, mode, unknown_is_filled, threshold = _CASES[key]
    cost, toward, reached = R.solve(field, weights, flags, sources, source_costs, cost_limit, mode, unknown_is_filled,
                                    threshold)
    cost.setflags(write=False)
    toward.setflags(write=False)
    return cost, toward, reached


_CASES = {}


def expected(field, weights, flags=0, sources=(), source_costs=None, cost_limit=R.NO_LIMIT, mode=R.OCCUPANCY,
             unknown_is_filled=True, threshold=0.0):
    """(cost, toward, num_reached) of the restatement, computed once per distinct case."""
    field = np.ascontiguousarray(field, dtype=np.float32)
    sources = np.asarray(sources, dtype=np.int64).reshape(-1)
    costs = None if source_costs is None else tuple(int(c) for c in source_costs)
    key = (field.shape, field.tobytes(), tuple(int(w) for w in weights), int(flags), tuple(int(s) for s in sources), costs,
           int(cost_limit), int(mode), bool(unknown_is_filled), float(threshold))
    if key not in _CASES:
        _CASES[key] = (field, tuple(int(w) for w in weights), int(flags), sources,
                       None if costs is None else np.asarray(costs, dtype=np.int64), int(cost_limit), int(mode),
                       bool(unknown_is_filled), float(threshold))
    return _expected(key)


@functools.lru_cache(maxsize=None)
def _expected_large(key):
    field, weights, flags, sources, source_costs = _LARGE[key]
    free = R.passable(field)
    cost = R.graph_cost(free, weights, flags, sources, source_costs)
    toward = R.toward(free, weights, flags, cost, sources, source_costs)
    cost.setflags(write=False)
    toward.setflags(write=False)
    return cost, toward, int(np.count_nonzero(cost != R.UNREACHED))


_LARGE = {}


def expected_large(field, weights, flags=0, sources=(), source_costs=None):
    """expected() for grids of hundreds of tiles (occupancy mode, no limit): the cost from R.graph_cost, which is scipy's
    Dijkstra where scipy imports and R.bellman_ford otherwise, `toward` by the same rule.  Computed once per case."""
    field = np.ascontiguousarray(field, dtype=np.float32)
    sources = np.asarray(sources, dtype=np.int64).reshape(-1)
    costs = None if source_costs is None else tuple(int(c) for c in source_costs)
    key = (field.shape, field.tobytes(), tuple(int(w) for w in weights), int(flags), tuple(int(s) for s in sources), costs)
    if key not in _LARGE:
        _LARGE[key] = (field, key[2], int(flags), sources, None if costs is None else np.asarray(costs, dtype=np.int64))
    return _expected_large(key)
