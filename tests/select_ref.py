"""CPU restatement of the cell selection (include/vgt_hip.h, vgt_hip_select_cells): the class of a value, the three
rules, and the selected cells in ascending linear index with their values and labels.

The 26-neighbour rule exists twice: `surface26_literal` is IsSurfaceIndex as the reference writes it
(S/occupancy_map.cpp:201-246: a loop over the clamped index ranges round the cell that returns at the first neighbour
that fires), `surface26` a vectorised form over shifted views.  tests/test_select_ref.py holds them against each other.
"""
import numpy as np

SELECT_ALL = 0
SELECT_SURFACE_26 = 1
SELECT_COMPONENT_SURFACE = 2
CLASS_ABOVE, CLASS_BELOW, CLASS_EQUAL, CLASS_UNORDERED = 1, 2, 4, 8


def classes(values, threshold):
    """uint8 grid: the class bit of every value against the threshold (float32 comparisons)."""
    v = np.asarray(values, dtype=np.float32)
    t = np.float32(threshold)
    with np.errstate(invalid="ignore"):
        above, below, equal = v > t, v < t, v == t
    out = np.full(v.shape, CLASS_UNORDERED, np.uint8)
    out[equal] = CLASS_EQUAL
    out[below] = CLASS_BELOW
    out[above] = CLASS_ABOVE
    return out


def surface26_literal(occ):
    """IsSurfaceIndex for every cell, as the reference's loop."""
    occ = np.asarray(occ, dtype=np.float32)
    nx, ny, nz = occ.shape
    half = np.float32(0.5)
    out = np.zeros(occ.shape, bool)

    def is_surface(x, y, z):
        our = occ[x, y, z]
        min_x, max_x = max(0, x - 1), min(nx - 1, x + 1)
        min_y, max_y = max(0, y - 1), min(ny - 1, y + 1)
        min_z, max_z = max(0, z - 1), min(nz - 1, z + 1)
        for xi in range(min_x, max_x + 1):
            for yi in range(min_y, max_y + 1):
                for zi in range(min_z, max_z + 1):
                    if (xi, yi, zi) == (x, y, z):
                        continue
                    other = occ[xi, yi, zi]
                    if our < half and other >= half:
                        return True
                    if our > half and other <= half:
                        return True
                    if our == half and other != half:
                        return True
        return False

    for x in range(nx):
        for y in range(ny):
            for z in range(nz):
                out[x, y, z] = is_surface(x, y, z)
    return out


def _any_neighbour(flag):
    """True where one of the up to 26 in-grid neighbours of a cell has the flag."""
    nx, ny, nz = flag.shape
    padded = np.zeros((nx + 2, ny + 2, nz + 2), bool)
    padded[1:-1, 1:-1, 1:-1] = flag
    out = np.zeros(flag.shape, bool)
    for dx in range(3):
        for dy in range(3):
            for dz in range(3):
                if (dx, dy, dz) != (1, 1, 1):
                    out |= padded[dx:dx + nx, dy:dy + ny, dz:dz + nz]
    return out


def surface26(occ):
    occ = np.asarray(occ, dtype=np.float32)
    half = np.float32(0.5)
    with np.errstate(invalid="ignore"):
        ge, le, ne = occ >= half, occ <= half, occ != half
        return ((occ < half) & _any_neighbour(ge)) | ((occ > half) & _any_neighbour(le)) | \
            ((occ == half) & _any_neighbour(ne))


def component_surface(labels):
    """The cell lies on a face of the grid or one of its six face neighbours has another label."""
    lab = np.asarray(labels, dtype=np.uint32)
    out = np.zeros(lab.shape, bool)
    for axis in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[axis], hi[axis] = slice(0, -1), slice(1, None)
        differs = lab[tuple(lo)] != lab[tuple(hi)]
        out[tuple(lo)] |= differs
        out[tuple(hi)] |= differs
        first = [slice(None)] * 3
        last = [slice(None)] * 3
        first[axis], last[axis] = 0, -1
        out[tuple(first)] = True
        out[tuple(last)] = True
    return out


def rule_mask(values, rule, labels=None):
    """The rule alone, before the classes: a bool grid."""
    if rule == SELECT_ALL:
        return np.ones(np.shape(values), bool)
    if rule == SELECT_SURFACE_26:
        return surface26(values)
    if rule == SELECT_COMPONENT_SURFACE:
        return component_surface(labels)
    raise ValueError("unknown rule")


def select(values, rule, class_mask, threshold=0.5, labels=None, rule_grid=None, class_grid=None):
    """(int32 indices ascending, float32 values, uint32 labels or None) of the selected cells.  rule_grid / class_grid:
    a rule_mask() / classes() computed before, for callers that run many class masks over one grid."""
    v = np.ascontiguousarray(values, dtype=np.float32)
    if rule == SELECT_SURFACE_26 and np.float32(threshold) != np.float32(0.5):
        raise ValueError("the 26-neighbour rule is defined for 0.5")
    if rule_grid is None:
        rule_grid = rule_mask(v, rule, labels)
    if class_grid is None:
        class_grid = classes(v, threshold)
    chosen = ((class_grid & np.uint8(class_mask)) != 0) & rule_grid
    indices = np.flatnonzero(chosen.reshape(-1)).astype(np.int32)
    lab = None if labels is None else np.ascontiguousarray(labels, dtype=np.uint32).reshape(-1)[indices]
    return indices, v.reshape(-1)[indices], lab
