"""CPU yardsticks of the component topology (beside components_ref.py; not a test module).

Written from the definition in include/vgt_hip.h, not from the reference's text.  Grid nx x ny x nz, `labels` as the
labelling writes them (1..N, 0 = no component), a cell outside the grid belongs to no component (-1).  For a label c
whose class is selected by component_types:
  V_c      = lattice vertices (i, j, k), 0 <= i <= nx etc., whose 8 cells (i-1..i, j-1..j, k-1..k) hold some cell of c
             and some cell not of c;
  exposed  = a lattice edge whose 4 cells hold some cell of c and some not; M3 / M5 / M6 = vertices of V_c with exactly
             3 / 5 / 6 exposed edges;
  surfaces = connected components of (V_c, exposed edges); voids = surfaces - 1;
  holes    = 1 + trunc((M5 + 2 M6 - M3) / 8) + voids, trunc = C division (toward zero).

`topology_literal` does this per label with Python sets and a queue walk; `topology_fast` with numpy over all (vertex,
label) pairs at once.  (The graph of the fast one is over those PAIRS -- a vertex carries up to 8 labels -- so it cannot
be a labelling of the vertex lattice by components_ref.fast_labels; it uses the same two back ends, scipy's
connected_components or min-label propagation, on the pair graph.)  Both return a structured array with one entry per
label 0..N: entry 0 and the entries of labels whose class is not selected are all zero.
"""
from collections import deque

import numpy as np

import components_ref as R

FIELDS = ("present", "num_holes", "num_voids", "num_surfaces", "m3", "m5", "m6", "num_surface_vertices")
TOPOLOGY = np.dtype([(name, np.int32) for name in FIELDS])

# the six edges at a vertex in the order of the result's bits (z-, z+, y-, y+, x-, x+): the direction and the 4 of the
# 8 cell offsets (dx, dy, dz in {-1, 0}) round the edge
_EDGES = []
for axis, sign in ((2, -1), (2, 1), (1, -1), (1, 1), (0, -1), (0, 1)):
    step = [0, 0, 0]
    step[axis] = sign
    cells = [(dx, dy, dz) for dx in (-1, 0) for dy in (-1, 0) for dz in (-1, 0)
             if (dx, dy, dz)[axis] == (-1 if sign < 0 else 0)]
    _EDGES.append((tuple(step), cells))


def trunc_div(a, b):
    """C's integer division (toward zero)."""
    q = abs(a) // abs(b)
    return q if (a >= 0) == (b >= 0) else -q


def class_bits(occ):
    occ = np.asarray(occ, dtype=np.float32)
    half = np.float32(0.5)
    with np.errstate(invalid="ignore"):
        return np.where(occ > half, R.FILLED_COMPONENTS, np.where(occ < half, R.EMPTY_COMPONENTS, R.UNKNOWN_COMPONENTS))


def _selected_labels(occ, labels, component_types, count):
    """bool [count + 1]: the class of the label's cells is selected (entry 0: False)."""
    selected = np.zeros(count + 1, dtype=bool)
    chosen = (class_bits(occ) & component_types) != 0
    lab = np.asarray(labels).reshape(-1)
    keep = chosen.reshape(-1) & (lab >= 1) & (lab <= count)
    selected[lab[keep]] = True
    return selected


def _entry(table, c, m3, m5, m6, vertices, surfaces):
    voids = surfaces - 1
    table[c] = (1, 1 + trunc_div(m5 + 2 * m6 - m3, 8) + voids, voids, surfaces, m3, m5, m6, vertices)


def topology_literal(occ, labels, component_types, count=None):
    labels = np.asarray(labels)
    nx, ny, nz = labels.shape
    count = int(labels.max()) if count is None else int(count)
    selected = _selected_labels(occ, labels, component_types, count)
    table = np.zeros(count + 1, dtype=TOPOLOGY)

    def comp(x, y, z):
        return int(labels[x, y, z]) if 0 <= x < nx and 0 <= y < ny and 0 <= z < nz else -1

    cells_of = {}
    for index in np.ndindex(nx, ny, nz):
        cells_of.setdefault(int(labels[index]), []).append(index)
    for c in range(1, count + 1):
        if not selected[c]:
            continue
        vertices = set()
        for x, y, z in cells_of.get(c, ()):
            for corner in ((x + a, y + b, z + d) for a in (0, 1) for b in (0, 1) for d in (0, 1)):
                if corner in vertices:
                    continue
                i, j, k = corner
                if any(comp(i + dx, j + dy, k + dz) != c for dx in (-1, 0) for dy in (-1, 0) for dz in (-1, 0)):
                    vertices.add(corner)
        exposed = {}
        m = {3: 0, 5: 0, 6: 0}
        for i, j, k in vertices:
            ends = []
            for step, cells in _EDGES:
                of_c = [comp(i + dx, j + dy, k + dz) == c for dx, dy, dz in cells]
                if any(of_c) and not all(of_c):
                    ends.append((i + step[0], j + step[1], k + step[2]))
            exposed[(i, j, k)] = ends
            if len(ends) in m:
                m[len(ends)] += 1
        surfaces = 0
        seen = set()
        for start in vertices:
            if start in seen:
                continue
            surfaces += 1
            seen.add(start)
            queue = deque([start])
            while queue:
                for end in exposed[queue.popleft()]:      # (KeyError = an exposed edge that leaves V_c)
                    if end not in seen:
                        seen.add(end)
                        queue.append(end)
        _entry(table, c, m[3], m[5], m[6], len(vertices), surfaces)
    return table


def _graph_components(n, rows, cols):
    """Component id per node of the undirected graph on n nodes (ids are arbitrary)."""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
        graph = coo_matrix((np.ones(rows.size, dtype=np.uint8), (rows, cols)), shape=(n, n))
        return connected_components(graph, directed=False)[1]
    except ImportError:
        comp = np.arange(n, dtype=np.int64)
        while True:
            before = comp.copy()
            np.minimum.at(comp, rows, comp[cols])
            np.minimum.at(comp, cols, comp[rows])
            comp = comp[comp]
            if np.array_equal(before, comp):
                return comp


def vertex_label_pairs(occ, labels, component_types, count=None):
    """The nodes of the definition: (vertex linear index over the (nx+1, ny+1, nz+1) lattice, label, 6-bit exposed-edge
    mask), sorted by (vertex, label)."""
    labels = np.asarray(labels)
    nx, ny, nz = labels.shape
    count = int(labels.max()) if count is None else int(count)
    selected = _selected_labels(occ, labels, component_types, count)
    padded = np.full((nx + 2, ny + 2, nz + 2), -1, dtype=np.int64)
    padded[1:-1, 1:-1, 1:-1] = labels

    def corner(dx, dy, dz):      # the cell at offset (dx, dy, dz) in {-1, 0} of every vertex
        return padded[1 + dx:nx + 2 + dx, 1 + dy:ny + 2 + dy, 1 + dz:nz + 2 + dz]
    offsets = [(dx, dy, dz) for dx in (-1, 0) for dy in (-1, 0) for dz in (-1, 0)]
    first = corner(*offsets[0])
    mixed = np.zeros(first.shape, dtype=bool)
    for o in offsets[1:]:
        mixed |= corner(*o) != first
    vertex = np.flatnonzero(mixed.reshape(-1))                       # only these can lie in any V_c
    around = np.stack([corner(*o).reshape(-1)[vertex] for o in offsets])   # [8, vertices]
    out_vertex, out_label, out_edges = [], [], []
    for q in range(8):
        lab = around[q]
        is_first = np.ones(lab.shape, dtype=bool)
        for r in range(q):
            is_first &= around[r] != lab
        ok = is_first & (lab >= 1) & (lab <= count)
        ok[ok] = selected[lab[ok]]
        same = around[:, ok] == lab[ok]                               # [8, nodes]: the cell is of the label
        edges = np.zeros(same.shape[1], dtype=np.int64)
        for bit, (_, cells) in enumerate(_EDGES):
            of_c = np.stack([same[offsets.index(cell)] for cell in cells])
            edges |= (of_c.any(axis=0) & ~of_c.all(axis=0)).astype(np.int64) << bit
        out_vertex.append(vertex[ok])
        out_label.append(lab[ok])
        out_edges.append(edges)
    v = np.concatenate(out_vertex)
    lab = np.concatenate(out_label)
    e = np.concatenate(out_edges)
    order = np.lexsort((lab, v))
    return v[order], lab[order], e[order], count, selected


def topology_fast(occ, labels, component_types, count=None):
    labels = np.asarray(labels)
    nx, ny, nz = labels.shape
    v, lab, edges, count, selected = vertex_label_pairs(occ, labels, component_types, count)
    table = np.zeros(count + 1, dtype=TOPOLOGY)
    n = v.size
    exposed = np.zeros(n, dtype=np.int64)
    for bit in range(6):
        exposed += (edges >> bit) & 1
    per_label = {k: np.bincount(lab[exposed == k], minlength=count + 1) for k in (3, 5, 6)}
    vertices = np.bincount(lab, minlength=count + 1)
    # the pair graph along the + edges (bits 1, 3, 5): the far node has the same label at the next vertex
    key = v * (count + 1) + lab                                        # ascending: the pairs are sorted
    stride = {1: 1, 3: nz + 1, 5: (ny + 1) * (nz + 1)}
    rows, cols = [], []
    for bit, step in stride.items():
        near = np.flatnonzero((edges >> bit) & 1)
        far = np.searchsorted(key, key[near] + step * (count + 1))
        assert np.array_equal(key[far], key[near] + step * (count + 1)), "an exposed edge leaves V_c"
        rows.append(near)
        cols.append(far)
    comp = _graph_components(n, np.concatenate(rows), np.concatenate(cols)) if n else np.zeros(0, dtype=np.int64)
    _, representative = np.unique(comp, return_index=True)
    surfaces = np.bincount(lab[representative], minlength=count + 1)
    present = selected & (vertices > 0)
    voids = surfaces - 1
    numerator = per_label[5] + 2 * per_label[6] - per_label[3]
    holes = 1 + np.sign(numerator) * (np.abs(numerator) // 8) + voids
    for name, values in (("present", present), ("num_holes", holes), ("num_voids", voids), ("num_surfaces", surfaces),
                         ("m3", per_label[3]), ("m5", per_label[5]), ("m6", per_label[6]),
                         ("num_surface_vertices", vertices)):
        table[name] = np.where(present, values, 0)
    return table


def labelled(occ, ids=None):
    """(occupancy float32, labels, count) with the labels of components_ref."""
    occ = np.asarray(occ, dtype=np.float32)
    labels, count = R.occupancy_labels_fast(occ, ids)
    return occ, labels, count


# ---- shapes with known answers: [(name, occupancy, {(class bit, a cell of the component): (holes, voids)})] ----
def _torus(shape, at, size=(7, 7, 2), hole=(3, 3)):
    occ = np.zeros(shape, np.float32)
    x, y, z = at
    occ[x:x + size[0], y:y + size[1], z:z + size[2]] = 1.0
    hx, hy = (size[0] - hole[0]) // 2, (size[1] - hole[1]) // 2
    occ[x + hx:x + hx + hole[0], y + hy:y + hy + hole[1], z:z + size[2]] = 0.0
    return occ


def known_answer_cases():
    nan = np.float32(np.nan)
    cases = []
    occ = np.zeros((12, 12, 12), np.float32)
    occ[3:8, 3:8, 3:8] = 1.0
    cases.append(("cube5_in_12", occ, {(3, 3, 3): (0, 0), (0, 0, 0): (0, 1)}))
    cases.append(("slab_with_a_hole", _torus((11, 11, 6), (2, 2, 2)), {(2, 2, 2): (1, 0)}))
    occ = np.zeros((11, 18, 6), np.float32)
    occ[2:9, 2:15, 2:4] = 1.0
    occ[4:7, 4:7, 2:4] = 0.0
    occ[4:7, 10:13, 2:4] = 0.0
    cases.append(("slab_with_two_holes", occ, {(2, 2, 2): (2, 0)}))
    occ = np.zeros((11, 11, 11), np.float32)
    occ[2:9, 2:9, 2:9] = 1.0
    occ[4:7, 4:7, 4:7] = 0.0
    cases.append(("shell_with_a_cavity", occ, {(2, 2, 2): (0, 1), (5, 5, 5): (0, 0), (0, 0, 0): (0, 1)}))
    cases.append(("filled_grid", np.ones((6, 6, 6), np.float32), {(0, 0, 0): (0, 0)}))
    occ = np.zeros((15, 15, 15), np.float32)
    occ[1:14, 1:14, 1:14] = 1.0
    occ[3:12, 3:12, 3:12] = 0.0
    occ[5:10, 5:10, 5:10] = 1.0
    occ[7, 7, 7] = 0.0
    # (outer shell: outside + inner surface = 1 void; the gap between the shells bounds two surfaces -> 1 void ...)
    cases.append(("nested_shells", occ, {(1, 1, 1): (0, 1), (3, 3, 3): (0, 1), (5, 5, 5): (0, 1), (7, 7, 7): (0, 0),
                                         (0, 0, 0): (0, 1)}))
    # two cavities in one block: voids 2
    occ = np.zeros((9, 13, 9), np.float32)
    occ[1:8, 1:12, 1:8] = 1.0
    occ[3:6, 3:5, 3:6] = 0.0
    occ[3:6, 8:10, 3:6] = 0.0
    cases.append(("two_cavities", occ, {(1, 1, 1): (0, 2)}))
    cases.append(("torus_touching_the_border", _torus((7, 9, 2), (0, 0, 0)), {(0, 0, 0): (1, 0)}))
    cases.append(("one_voxel", np.ones((1, 1, 1), np.float32), {(0, 0, 0): (0, 0)}))
    # two voxels that share only an edge, joined by a third path: the numerator is not a multiple of 8
    occ = np.zeros((5, 5, 4), np.float32)
    occ[1, 1, 1] = occ[2, 2, 1] = 1.0
    occ[1, 1, 2] = occ[2, 1, 2] = occ[2, 2, 2] = 1.0
    cases.append(("pinched_pair", occ, {}))
    cases.append(("all_unknown", np.full((4, 3, 5), 0.5, np.float32), {(0, 0, 0): (0, 0)}))
    occ = np.zeros((4, 4, 4), np.float32)
    occ[1, 1, 1] = occ[1, 1, 2] = nan
    occ[2, 2, 2] = 1.0
    cases.append(("nan_cells", occ, {(2, 2, 2): (0, 0), (1, 1, 1): (0, 0), (1, 1, 2): (0, 0)}))
    return cases


def hand_cases():
    """[(name, occupancy, object ids)]: the known-answer shapes and the labelling's own hand cases."""
    cases = [(name, occ, np.zeros(occ.shape, np.uint32)) for name, occ, _ in known_answer_cases()]
    cases += [(name, occ, np.zeros(occ.shape, np.uint32)) for name, occ, _, _ in R.hand_cases()]
    return cases


def tables_equal(got, want):
    got = np.asarray(got)
    want = np.asarray(want)
    return got.shape == want.shape and all(
        got[name].dtype == np.int32 and np.array_equal(got[name], want[name]) for name in FIELDS)
