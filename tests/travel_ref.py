"""The definition of vgt_hip_travel_cost (include/vgt_hip.h) restated twice in numpy: a heap Dijkstra written as a loop
and a vectorised Bellman-Ford of shifted-array minima iterated to the fixed point; the `toward` rule; the path follower
of vgt_hip_trace_paths.  Nothing here is shared with the library."""
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
    """uint32 cost by shifted-array minima iterated to the fixed point, in int64 with a large 'infinity'."""
    inf = np.int64(1) << 40
    cost = np.full(free.shape, inf, dtype=np.int64)
    flat = cost.reshape(-1)
    for s, c0 in _contributing(free, sources, source_costs, cost_limit).items():
        flat[s] = min(flat[s], c0)
    moves = allowed_moves(free, weights, flags)
    while True:
        new = cost.copy()
        for d, ok in moves.items():
            w = int(weights[sum(1 for v in d if v) - 1])
            cand = _shifted(cost, d, inf) + w
            cand[~ok | (cand > cost_limit)] = inf
            np.minimum(new, cand, out=new)
        if np.array_equal(new, cost):
            break
        cost = new
    out = np.where(cost >= inf, UNREACHED, cost).astype(np.uint32)
    return out


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
