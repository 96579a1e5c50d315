"""The definition of vgt_hip_travel_cost (include/vgt_hip.h) restated twice in numpy: a heap Dijkstra written as a loop
and a vectorised Bellman-Ford of shifted-array minima iterated to the fixed point; the `toward` rule; the path follower
of vgt_hip_trace_paths.  For grids of hundreds of tiles, graph_cost (scipy's Dijkstra when scipy imports).  tile_rounds
models the rounds in which the library relaxes tiles, to choose inputs and to say what they exercise.  Nothing here is
shared with the library."""
import heapq
import itertools

import numpy as np

UNREACHED = 0xffffffff
NO_LIMIT = 0xfffffffe
OCCUPANCY, SDF_ABOVE = 0, 1
NO_CORNER_CUTTING = 1
TRACE_OK, TRACE_UNREACHED, TRACE_TRUNCATED, TRACE_INVALID = 0, 1, 2, 3

# (dx, dy, dz) ascending lexicographically over -1, 0, 1, without the zero offset: the order of `toward`
OFFSETS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d != (0, 0, 0)]


def passable(field, mode=OCCUPANCY, unknown_is_filled=True, threshold=0.0):
    """bool (nx, ny, nz): the cells vgt_hip_cast_segments would not call a hit."""
    f = np.asarray(field, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        if mode == OCCUPANCY:
            blocked = f > np.float32(0.5)
            if unknown_is_filled:
                blocked |= f == np.float32(0.5)
        else:
            blocked = f.astype(np.float64) <= np.float64(threshold)
    return ~blocked


def _move_ok(free, a, d, strict):
    """Is the move a -> a + d allowed (the class being enabled)?  a: (x, y, z) of a passable cell."""
    shape = free.shape
    b = (a[0] + d[0], a[1] + d[1], a[2] + d[2])
    if not all(0 <= b[i] < shape[i] for i in range(3)):
        return False
    if not free[b]:
        return False
    if strict:
        for s in itertools.product(*[(0, d[i]) if d[i] else (0,) for i in range(3)]):
            if not free[a[0] + s[0], a[1] + s[1], a[2] + s[2]]:
                return False
    return True


def _contributing(free, sources, source_costs, cost_limit):
    """{cell: least initial cost} of the sources that contribute."""
    n = free.size
    flat = free.reshape(-1)
    init = {}
    for i, s in enumerate(np.asarray(sources, dtype=np.int64).reshape(-1)):
        c0 = 0 if source_costs is None else int(source_costs[i])
        if s < 0 or s >= n or not flat[s] or c0 > cost_limit:
            continue
        init[int(s)] = min(init.get(int(s), c0), c0)
    return init


def dijkstra(free, weights, flags, sources, source_costs=None, cost_limit=NO_LIMIT):
    """uint32 cost (nx, ny, nz) by a heap Dijkstra, Python integers throughout (no wrap-around)."""
    shape = free.shape
    strict = bool(flags & NO_CORNER_CUTTING)
    cost = {}
    heap = [(c0, s) for s, c0 in _contributing(free, sources, source_costs, cost_limit).items()]
    heapq.heapify(heap)
    while heap:
        c, a = heapq.heappop(heap)
        if a in cost:
            continue
        cost[a] = c
        xyz = np.unravel_index(a, shape)
        xyz = (int(xyz[0]), int(xyz[1]), int(xyz[2]))
        for d in OFFSETS:
            w = int(weights[sum(1 for v in d if v) - 1])
            if w == 0 or c + w > cost_limit or not _move_ok(free, xyz, d, strict):
                continue
            b = int(np.ravel_multi_index((xyz[0] + d[0], xyz[1] + d[1], xyz[2] + d[2]), shape))
            if b not in cost:
                heapq.heappush(heap, (c + w, b))
    out = np.full(free.size, UNREACHED, dtype=np.uint32)
    for a, c in cost.items():
        out[a] = c
    return out.reshape(shape)


def _shifted(a, d, fill):
    """out[p] = a[p + d] where p + d is in the grid, else fill."""
    out = np.full_like(a, fill)
    src, dst = [], []
    for i in range(3):
        n = a.shape[i]
        if d[i] == 0:
            src.append(slice(0, n)), dst.append(slice(0, n))
        elif d[i] > 0:
            src.append(slice(1, n)), dst.append(slice(0, n - 1))
        else:
            src.append(slice(0, n - 1)), dst.append(slice(1, n))
    out[tuple(dst)] = a[tuple(src)]
    return out


def allowed_moves(free, weights, flags):
    """{d: bool (nx, ny, nz)}: the move c -> c + d is allowed, for the enabled classes."""
    strict = bool(flags & NO_CORNER_CUTTING)
    out = {}
    for d in OFFSETS:
        if int(weights[sum(1 for v in d if v) - 1]) == 0:
            continue
        ok = free & _shifted(free, d, False)
        if strict:
            for s in itertools.product(*[(0, d[i]) if d[i] else (0,) for i in range(3)]):
                ok &= _shifted(free, s, False)
        out[d] = ok
    return out


def bellman_ford(free, weights, flags, sources, source_costs=None, cost_limit=NO_LIMIT):
    """uint32 cost by shifted-array minima iterated to the fixed point, in int64 with a large 'infinity'.  Every sweep
    takes all its candidates from the previous sweep's field; it covers the bounding box, grown by one cell, of the cells
    the previous sweep lowered, since no other cell has a neighbour that changed (a long corridor needs thousands of
    sweeps that each lower one cell)."""
    shape = free.shape
    inf = np.int64(1) << 40
    padded = np.full(tuple(s + 2 for s in shape), inf, dtype=np.int64)  # a rim of 'infinity' round the grid
    cost = padded[1:-1, 1:-1, 1:-1]
    for s, c0 in _contributing(free, sources, source_costs, cost_limit).items():
        xyz = np.unravel_index(s, shape)
        cost[xyz] = min(cost[xyz], c0)
    moves = allowed_moves(free, weights, flags)
    lo, hi = (0, 0, 0), shape
    while True:
        box = tuple(slice(lo[i], hi[i]) for i in range(3))
        old = cost[box]
        new = old.copy()
        for d, ok in moves.items():
            w = int(weights[sum(1 for v in d if v) - 1])
            cand = padded[tuple(slice(lo[i] + 1 + d[i], hi[i] + 1 + d[i]) for i in range(3))] + w
            cand[~ok[box] | (cand > cost_limit)] = inf
            np.minimum(new, cand, out=new)
        lowered = np.nonzero(new < old)
        if lowered[0].size == 0:
            break
        cost[box] = new
        lo, hi = (tuple(max(lo[i] + int(lowered[i].min()) - 1, 0) for i in range(3)),
                  tuple(min(lo[i] + int(lowered[i].max()) + 2, shape[i]) for i in range(3)))
    out = np.where(cost >= inf, UNREACHED, cost).astype(np.uint32)
    return out


def graph_cost(free, weights, flags, sources, source_costs=None, cost_limit=NO_LIMIT):
    """uint32 cost for grids too large for the two forms above: the allowed moves as a sparse directed graph and scipy's
    Dijkstra from one extra node joined to every contributing source, where scipy imports; bellman_ford otherwise."""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import dijkstra as graph_dijkstra
    except ImportError:
        return bellman_ford(free, weights, flags, sources, source_costs, cost_limit)
    n = free.size
    index = np.arange(n, dtype=np.int64).reshape(free.shape)
    rows, cols, vals = [], [], []
    for d, ok in allowed_moves(free, weights, flags).items():
        rows.append(index[ok])
        cols.append(_shifted(index, d, -1)[ok])
        vals.append(np.full(rows[-1].size, float(weights[sum(1 for v in d if v) - 1])))
    # the extra node n; its edges carry init + 1 (an entry of 0 would not be an edge), taken off again below
    init = _contributing(free, sources, source_costs, cost_limit)
    rows.append(np.full(len(init), n, dtype=np.int64))
    cols.append(np.fromiter(init.keys(), dtype=np.int64, count=len(init)))
    vals.append(np.fromiter(init.values(), dtype=np.float64, count=len(init)) + 1.0)
    graph = coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n + 1, n + 1)).tocsr()
    dist = graph_dijkstra(graph, directed=True, indices=[n], min_only=True)[:n] - 1.0  # (integers below 2^53: exact)
    # (every prefix of a least-cost path within the limit is within the limit: cutting afterwards is the definition)
    reached = np.isfinite(dist) & (dist <= cost_limit)
    out = np.full(n, UNREACHED, dtype=np.uint32)
    out[reached] = dist[reached].astype(np.uint32)
    return out.reshape(free.shape)


def tile_rounds(free, weights, flags, sources, source_costs=None, cost_limit=NO_LIMIT, tile=(8, 8, 16)):
    """A model of HOW the library reaches the cost field, not of the field: tiles relaxed in rounds.  In
    a round every flagged tile reads its cells and a one-cell halo from a snapshot of the previous round's costs, relaxes
    its own cells to the fixed point, and stores the cells it lowered; a lowered cell on a face, an edge or a corner of
    its tile flags, for the next round, the neighbouring tiles that see it in their halo; a contributing source flags
    its tile and those neighbours for the first round.  -> (rounds, cost uint32, writes, most_active): the number of
    rounds with a flagged tile, the field after the last, per cell the number of rounds that lowered it, and the most
    tiles flagged in one round.  The device may see a value stored in the same round and then needs fewer rounds, so
    its count is never compared for equality; this serves to choose inputs and to state what they exercise."""
    shape = free.shape
    inf = np.int64(1) << 40
    counts = tuple(-(-shape[i] // tile[i]) for i in range(3))
    moves = allowed_moves(free, weights, flags)
    padded = np.full(tuple(s + 2 for s in shape), inf, dtype=np.int64)  # a rim of 'infinity': halo cells off the grid
    cost = padded[1:-1, 1:-1, 1:-1]
    writes = np.zeros(shape, dtype=np.int64)

    def flag_neighbours(flagged, t, lowered, with_itself):
        """`lowered`: bool over the cells of tile t (clipped to the grid)."""
        where = np.nonzero(lowered)
        if where[0].size == 0:
            return
        for s in itertools.product((-1, 0, 1), repeat=3):
            if s == (0, 0, 0) and not with_itself:
                continue
            other = tuple(t[i] + s[i] for i in range(3))
            if not all(0 <= other[i] < counts[i] for i in range(3)):
                continue
            on = np.ones(where[0].size, dtype=bool)
            for i in range(3):
                if s[i]:
                    on &= where[i] == (0 if s[i] < 0 else tile[i] - 1)
            if on.any():
                flagged.add(other)

    flagged = set()
    for s, c0 in _contributing(free, sources, source_costs, cost_limit).items():
        xyz = tuple(int(v) for v in np.unravel_index(s, shape))
        cost[xyz] = min(cost[xyz], c0)
        t = tuple(xyz[i] // tile[i] for i in range(3))
        one = np.zeros(tile, dtype=bool)
        one[tuple(xyz[i] - t[i] * tile[i] for i in range(3))] = True
        flag_neighbours(flagged, t, one, True)

    rounds = most_active = 0
    while flagged:
        rounds += 1
        most_active = max(most_active, len(flagged))
        snapshot = padded.copy()
        flagged_next = set()
        for t in sorted(flagged):
            lo = tuple(t[i] * tile[i] for i in range(3))
            hi = tuple(min(lo[i] + tile[i], shape[i]) for i in range(3))
            own_box = tuple(slice(lo[i], hi[i]) for i in range(3))
            local = snapshot[tuple(slice(lo[i], hi[i] + 2) for i in range(3))].copy()  # the tile and its halo
            own = local[1:-1, 1:-1, 1:-1]
            before = own.copy()
            steps = [(local[tuple(slice(1 + d[i], 1 + d[i] + hi[i] - lo[i]) for i in range(3))],
                      int(weights[sum(1 for v in d if v) - 1]), ~ok[own_box]) for d, ok in moves.items()]
            while True:
                new = own.copy()
                for neighbour, w, barred in steps:  # (`neighbour` is a view of `local`: it follows `own`)
                    cand = neighbour + w
                    cand[barred | (cand > cost_limit)] = inf
                    np.minimum(new, cand, out=new)
                if np.array_equal(new, own):
                    break
                own[...] = new
            lowered = own < before
            cost[own_box][lowered] = own[lowered]
            writes[own_box] += lowered
            flag_neighbours(flagged_next, t, lowered, False)
        flagged = flagged_next
    out = np.where(cost >= inf, UNREACHED, cost).astype(np.uint32)
    return rounds, out, writes, most_active


def toward(free, weights, flags, cost, sources, source_costs=None, cost_limit=NO_LIMIT):
    """int32 toward (nx, ny, nz) from a converged cost field: the rule of the header."""
    shape = cost.shape
    n = cost.size
    c64 = np.where(cost == UNREACHED, np.int64(1) << 40, cost.astype(np.int64))
    out = np.full(shape, -1, dtype=np.int64)
    index = np.arange(n, dtype=np.int64).reshape(shape)
    reached = cost != UNREACHED
    moves = allowed_moves(free, weights, flags)
    for d in reversed(OFFSETS):  # the first in ascending order wins: write the later ones first
        if d not in moves:
            continue
        w = int(weights[sum(1 for v in d if v) - 1])
        match = reached & moves[d] & (_shifted(c64, d, np.int64(1) << 41) + w == c64)
        out[match] = _shifted(index, d, -1)[match]
    flat, cflat = out.reshape(-1), cost.reshape(-1)
    for s, c0 in _contributing(free, sources, source_costs, cost_limit).items():
        if int(cflat[s]) == c0:
            flat[s] = s
    return out.astype(np.int32)


def solve(field, weights, flags=0, sources=(), source_costs=None, cost_limit=NO_LIMIT, mode=OCCUPANCY,
          unknown_is_filled=True, threshold=0.0, free=None):
    """(cost uint32, toward int32, num_reached) of the definition (Bellman-Ford form)."""
    if free is None:
        free = passable(field, mode, unknown_is_filled, threshold)
    cost = bellman_ford(free, weights, flags, sources, source_costs, cost_limit)
    tw = toward(free, weights, flags, cost, sources, source_costs, cost_limit)
    return cost, tw, int(np.count_nonzero(cost != UNREACHED))


def trace_paths(toward_field, starts, max_cells, fill=-1):
    """(paths int32 [N, max_cells] with `fill` in the untouched slots, lengths int32, status uint8)."""
    t = np.asarray(toward_field, dtype=np.int64).reshape(-1)
    n = t.size
    starts = np.asarray(starts, dtype=np.int64).reshape(-1)
    paths = np.full((starts.size, max_cells), fill, dtype=np.int32)
    lengths = np.zeros(starts.size, dtype=np.int32)
    status = np.zeros(starts.size, dtype=np.uint8)
    for i, cur in enumerate(starts):
        length, result = 0, TRACE_INVALID
        while 0 <= cur < n:
            nxt = t[cur]
            if nxt < -1 or nxt >= n:
                break
            if nxt == -1:
                if length == 0:
                    result = TRACE_UNREACHED
                break
            paths[i, length] = cur
            length += 1
            if nxt == cur:
                result = TRACE_OK
                break
            if length == max_cells:
                result = TRACE_TRUNCATED
                break
            cur = nxt
        lengths[i], status[i] = length, result
    return paths, lengths, status
