"""CPU yardsticks of the component labelling (beside sdf_conversion_ref.py; not a test module).

`flood_fill_labels` restates the reference's topology_computation::ComputeConnectedComponents +
MarkConnectedComponent (include/voxelized_geometry_tools/topology_computation.hpp:59-196) literally: start cells in
X-major / Z-fastest order, a FIFO queue, the six neighbours in the order -X +X -Y +Y -Z +Z, the "still unlabelled" test
before the predicate.  `fast_labels` is a quick equivalent for large grids; the tests trust it only after showing it
equal to the flood fill on every small case.  The three predicates and the component-surface rule are numpy expressions
of the reference's lambdas.
"""
from collections import deque

import numpy as np

FILLED_COMPONENTS, EMPTY_COMPONENTS, UNKNOWN_COMPONENTS = 0x01, 0x02, 0x04
_NEIGHBOURS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


def flood_fill_labels(active, connected):
    """active: bool [nx, ny, nz] (False = the reference's get_component_fn returns -1);
    connected(a, b): predicate on two index triples.  -> (uint32 labels, count)."""
    active = np.asarray(active, dtype=bool)
    nx, ny, nz = active.shape
    labels = np.zeros(active.shape, dtype=np.uint32)
    component = np.where(active, 0, -1).astype(np.int64)   # what get_component_fn returns
    count = 0
    for x in range(nx):
        for y in range(ny):
            for z in range(nz):
                if component[x, y, z] != 0:
                    continue
                count += 1
                queue = deque([(x, y, z)])
                queued = {(x, y, z)}
                while queue:
                    cur = queue.popleft()
                    component[cur] = count
                    labels[cur] = count
                    for dx, dy, dz in _NEIGHBOURS:
                        nb = (cur[0] + dx, cur[1] + dy, cur[2] + dz)
                        if not (0 <= nb[0] < nx and 0 <= nb[1] < ny and 0 <= nb[2] < nz):
                            continue
                        if component[nb] == 0 and connected(cur, nb) and nb not in queued:
                            queued.add(nb)
                            queue.append(nb)
    return labels, count


# ---- predicates as functions of two index triples (for the flood fill) ----
def occupancy_connected(occ, ids=None):
    """occupancy_component_map.cpp:457-481; with ids: tagged_object_occupancy_component_map.cpp:700-745 without
    connect_across_objects."""
    occ = np.asarray(occ, dtype=np.float32)
    half = np.float32(0.5)

    def connected(a, b):
        oa, ob = occ[a], occ[b]
        same = (oa > half and ob > half) or (oa < half and ob < half) or (oa == half and ob == half)
        return bool(same and (ids is None or ids[a] == ids[b]))
    return connected


def segment_active(occ, ids, extrema):
    """tagged_object_occupancy_component_map.cpp:821-853."""
    occ = np.asarray(occ, dtype=np.float32)
    return ((occ < np.float32(0.5)) | (np.asarray(ids) > 0)) & ~np.isinf(extrema).any(axis=-1)


def _distance(ea, eb):
    d = ea - eb
    with np.errstate(invalid="ignore"):
        return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def segment_connected(ids, extrema, threshold):
    """:796-820 (the distance in double as sqrt((dx*dx + dy*dy) + dz*dz))."""
    def connected(a, b):
        return bool(ids[a] == ids[b] and _distance(extrema[a], extrema[b]) < threshold)
    return connected


# ---- the same as edge arrays (for fast_labels) ----
def _axis_pairs(shape, axis):
    lo = [slice(None)] * 3
    hi = [slice(None)] * 3
    lo[axis] = slice(0, shape[axis] - 1)
    hi[axis] = slice(1, shape[axis])
    return tuple(lo), tuple(hi)


def occupancy_edges(occ, ids=None):
    """Per axis: bool array over the pairs (cell, cell + 1 along the axis) = connected."""
    occ = np.asarray(occ, dtype=np.float32)
    half = np.float32(0.5)
    with np.errstate(invalid="ignore"):
        cls = np.where(occ > half, 0, np.where(occ < half, 1, np.where(occ == half, 2, 3)))
    edges = []
    for axis in range(3):
        lo, hi = _axis_pairs(occ.shape, axis)
        e = (cls[lo] == cls[hi]) & (cls[lo] != 3)
        if ids is not None:
            e &= ids[lo] == ids[hi]
        edges.append(e)
    return edges


def segment_edges(occ, ids, extrema, threshold):
    active = segment_active(occ, ids, extrema)
    edges = []
    for axis in range(3):
        lo, hi = _axis_pairs(active.shape, axis)
        with np.errstate(invalid="ignore"):
            near = _distance(np.where(active[lo][..., None], extrema[lo], 0.0),
                             np.where(active[hi][..., None], extrema[hi], 0.0)) < threshold
        edges.append(active[lo] & active[hi] & (ids[lo] == ids[hi]) & near)
    return edges


def segment_edge_distances(occ, ids, extrema):
    """Distances of all face-adjacent active pairs with equal ids (what the threshold is compared with)."""
    active = segment_active(occ, ids, extrema)
    out = []
    for axis in range(3):
        lo, hi = _axis_pairs(active.shape, axis)
        pair = active[lo] & active[hi] & (ids[lo] == ids[hi])
        out.append(_distance(extrema[lo][pair], extrema[hi][pair]))
    return np.concatenate(out) if out else np.zeros(0)


def fast_labels(active, edges):
    """Components of the graph (active cells, `edges` per axis as of occupancy_edges), numbered in ascending order of
    their smallest linear index.  scipy's sparse connected_components when importable, else min-label propagation."""
    active = np.asarray(active, dtype=bool)
    shape = active.shape
    n = active.size
    index = np.arange(n, dtype=np.int64).reshape(shape)
    rows, cols = [], []
    for axis in range(3):
        lo, hi = _axis_pairs(shape, axis)
        e = edges[axis] & active[lo] & active[hi]
        rows.append(index[lo][e])
        cols.append(index[hi][e])
    rows = np.concatenate(rows)
    cols = np.concatenate(cols)
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        graph = coo_matrix((np.ones(rows.size, dtype=np.uint8), (rows, cols)), shape=(n, n))
        _, comp = connected_components(graph, directed=False)
    except ImportError:
        comp = np.arange(n, dtype=np.int64)
        while True:
            before = comp.copy()
            np.minimum.at(comp, rows, comp[cols])
            np.minimum.at(comp, cols, comp[rows])
            comp = comp[comp]
            if np.array_equal(before, comp):
                break
    flat_active = active.reshape(-1)
    # renumber by first linear index among the active cells
    act_idx = np.flatnonzero(flat_active)
    _, first, inverse = np.unique(comp[act_idx], return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")                         # components in order of first appearance
    rank = np.empty(order.size, dtype=np.int64)
    rank[order] = np.arange(1, order.size + 1)
    labels = np.zeros(n, dtype=np.uint32)
    labels[act_idx] = rank[inverse.reshape(-1)]
    return labels.reshape(shape), int(order.size)


def occupancy_labels_fast(occ, ids=None):
    occ = np.asarray(occ, dtype=np.float32)
    return fast_labels(np.ones(occ.shape, dtype=bool), occupancy_edges(occ, ids))


def occupancy_labels_flood(occ, ids=None):
    occ = np.asarray(occ, dtype=np.float32)
    return flood_fill_labels(np.ones(occ.shape, dtype=bool), occupancy_connected(occ, ids))


def segment_labels_fast(occ, ids, extrema, threshold):
    return fast_labels(segment_active(occ, ids, extrema), segment_edges(occ, ids, extrema, threshold))


def segment_labels_flood(occ, ids, extrema, threshold):
    return flood_fill_labels(segment_active(occ, ids, extrema), segment_connected(ids, extrema, threshold))


def surface_mask(occ, labels, component_types):
    """occupancy_component_map.cpp:290-350 (six face neighbours) and :531-567 (class selection; the final `else` makes
    NaN "unknown")."""
    occ = np.asarray(occ, dtype=np.float32)
    labels = np.asarray(labels)
    half = np.float32(0.5)
    with np.errstate(invalid="ignore"):
        bit = np.where(occ > half, FILLED_COMPONENTS, np.where(occ < half, EMPTY_COMPONENTS, UNKNOWN_COMPONENTS))
    selected = (bit & component_types) != 0
    surface = np.zeros(occ.shape, dtype=bool)
    for axis in range(3):
        first = [slice(None)] * 3
        last = [slice(None)] * 3
        first[axis] = 0
        last[axis] = -1
        surface[tuple(first)] = True
        surface[tuple(last)] = True
        lo, hi = _axis_pairs(occ.shape, axis)
        differs = labels[lo] != labels[hi]
        surface[lo] |= differs
        surface[hi] |= differs
    return selected & surface


# ---- the cases the tests share ----
def hand_cases():
    """[(name, occupancy, expected labels, expected count)] derived by hand."""
    nan = np.float32(np.nan)
    cases = []
    cases.append(("single", np.zeros((1, 1, 1), np.float32), np.ones((1, 1, 1), np.uint32), 1))
    # filled centre of a 3x3x3 grid: the empty shell holds index 0 -> 1, the centre -> 2
    occ = np.zeros((3, 3, 3), np.float32)
    occ[1, 1, 1] = 1.0
    want = np.ones((3, 3, 3), np.uint32)
    want[1, 1, 1] = 2
    cases.append(("filled_centre", occ, want, 2))
    # two filled boxes that touch along an edge only (diagonal neighbours): not connected.  4x4x1 grid, boxes
    # [0:2, 0:2] and [2:4, 2:4]; the two empty quadrants touch along an edge only as well.
    occ = np.zeros((4, 4, 1), np.float32)
    occ[0:2, 0:2] = 1.0
    occ[2:4, 2:4] = 1.0
    want = np.zeros((4, 4, 1), np.uint32)
    want[0:2, 0:2] = 1     # holds linear index 0
    want[0:2, 2:4] = 2     # first cell (0, 2, 0) = index 2
    want[2:4, 0:2] = 3     # first cell (2, 0, 0) = index 8
    want[2:4, 2:4] = 4     # first cell (2, 2, 0) = index 10
    cases.append(("boxes_touching_along_an_edge", occ, want, 4))
    # an unknown (0.5) shell between an empty outside and an empty inside: three components, three classes of order
    occ = np.zeros((5, 5, 5), np.float32)
    occ[1:4, 1:4, 1:4] = 0.5
    occ[2, 2, 2] = 0.0
    want = np.ones((5, 5, 5), np.uint32)
    want[1:4, 1:4, 1:4] = 2
    want[2, 2, 2] = 3
    cases.append(("unknown_shell", occ, want, 3))
    # a NaN cell connects to nothing: a component of its own
    occ = np.zeros((1, 1, 5), np.float32)
    occ[0, 0, 2] = nan
    cases.append(("nan_cell", occ, np.array([1, 1, 2, 3, 3], np.uint32).reshape(1, 1, 5), 3))
    # numbering follows the first linear index, not the size: the component with index 0 is one cell
    occ = np.zeros((2, 2, 3), np.float32)
    occ[0, 0, 0] = 1.0
    want = np.full((2, 2, 3), 2, np.uint32)
    want[0, 0, 0] = 1
    cases.append(("numbering_order", occ, want, 2))
    return cases


OCCUPANCY_VALUES = np.array([0.0, 0.25, 0.5, 0.75, 1.0, np.nan], dtype=np.float32)


def random_small_grids(count=200, seed=20240611):
    """[(occupancy, object ids)]: extents 1..12 per axis, occupancies from OCCUPANCY_VALUES, ids in 0..3."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        shape = tuple(int(v) for v in rng.integers(1, 13, size=3))
        # a few values per grid so that components larger than one cell exist
        palette = rng.choice(OCCUPANCY_VALUES, size=int(rng.integers(1, 7)))
        occ = rng.choice(palette, size=shape).astype(np.float32)
        ids = rng.integers(0, 4, size=shape).astype(np.uint32)
        if rng.random() < 0.5:   # blocky ids: objects larger than one cell
            ids = np.repeat(np.repeat(np.repeat(ids, 3, 0), 3, 1), 3, 2)[:shape[0], :shape[1], :shape[2]].copy()
        out.append((occ, ids))
    return out


def lattice_extrema(shape, resolution, seed, inf_share=0.1, spread=3):
    """A synthetic local-extrema map: every entry a lattice point (k + 0.5) * resolution near the cell, a seeded share of
    +inf triples.  Distances between entries are resolution * sqrt(integer)."""
    rng = np.random.default_rng(seed)
    grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), axis=-1)
    # blocky offsets: neighbouring cells often share an extremum
    coarse = rng.integers(-spread, spread + 1, size=tuple((s + 3) // 4 for s in shape) + (3,))
    offsets = np.repeat(np.repeat(np.repeat(coarse, 4, 0), 4, 1), 4, 2)[:shape[0], :shape[1], :shape[2]]
    jitter = rng.integers(0, 2, size=tuple(shape) + (3,)) * (rng.random(tuple(shape) + (1,)) < 0.3)
    cells = (grid // 4) * 4 + offsets + jitter
    extrema = (cells.astype(np.float64) + 0.5) * float(resolution)
    extrema[rng.random(shape) < inf_share] = np.inf
    return extrema


def assert_threshold_is_clear(occ, ids, extrema, threshold):
    """The tests' condition on a threshold: no face-adjacent active pair's distance within a relative 1e-9 of it."""
    d = segment_edge_distances(occ, ids, extrema)
    d = d[np.isfinite(d)]
    assert not np.any(np.abs(d - threshold) <= 1e-9 * threshold), "a pair's distance lies at the threshold"
