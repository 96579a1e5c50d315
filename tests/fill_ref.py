"""CPU yardstick of vgt_hip_fill_enclosed (beside components_ref.py; not a test module).

The definition of include/vgt_hip.h restated in numpy: filled = occupancy > 0.5 or (unknown_is_filled and == 0.5),
passable = not filled (NaN included); outside = the passable cells that a chain of face-adjacent passable cells joins to
a passable cell on a face of the grid; every other passable cell becomes 1.0 and nothing else changes.  Two routes to
"outside", which test_fill_ref.py shows equal: the components of the passable cells (components_ref.fast_labels) and
growing outward from the border by repeated face-neighbour propagation.  scipy is not needed by either.
"""
import numpy as np

import components_ref as R
import topology_ref as T


def passable(occ, unknown_is_filled=True):
    occ = np.asarray(occ, dtype=np.float32)
    half = np.float32(0.5)
    with np.errstate(invalid="ignore"):
        filled = (occ > half) | ((occ == half) if unknown_is_filled else False)
    return ~filled


def border(shape):
    """bool: the cell's index is 0 or n - 1 on some axis."""
    b = np.zeros(shape, dtype=bool)
    for axis in range(3):
        first = [slice(None)] * 3
        last = [slice(None)] * 3
        first[axis] = 0
        last[axis] = -1
        b[tuple(first)] = True
        b[tuple(last)] = True
    return b


def outside_by_labels(free):
    """Components of the passable cells (every face-adjacent passable pair is an edge); outside = the components that
    hold a border cell."""
    free = np.asarray(free, dtype=bool)
    edges = [np.ones(tuple(s - (1 if a == axis else 0) for a, s in enumerate(free.shape)), dtype=bool)
             for axis in range(3)]
    labels, count = R.fast_labels(free, edges)
    is_outside = np.zeros(count + 1, dtype=bool)
    is_outside[labels[border(free.shape) & free]] = True
    is_outside[0] = False
    return is_outside[labels]


def outside_by_growing(free):
    """Start from the passable border cells and add passable face neighbours until nothing changes."""
    free = np.asarray(free, dtype=bool)
    out = border(free.shape) & free
    while True:
        grown = out.copy()
        for axis in range(3):
            lo, hi = R._axis_pairs(free.shape, axis)
            grown[hi] |= out[lo]
            grown[lo] |= out[hi]
        grown &= free
        if np.array_equal(grown, out):
            return out
        out = grown


def outside_quick(free):
    """For large grids: scipy.ndimage.label (face structure) where scipy imports, else outside_by_labels.  The tests
    trust it only after showing it equal to the two above."""
    try:
        from scipy import ndimage
    except ImportError:
        return outside_by_labels(free)
    free = np.asarray(free, dtype=bool)
    labels, count = ndimage.label(free)
    is_outside = np.zeros(count + 1, dtype=bool)
    is_outside[labels[border(free.shape) & free]] = True
    is_outside[0] = False
    return is_outside[labels]


def enclosed(occ, unknown_is_filled=True, outside=outside_by_labels):
    free = passable(occ, unknown_is_filled)
    return free & ~outside(free)


def fill(occ, unknown_is_filled=True, outside=outside_by_labels):
    """-> (the filled map: a copy in which only the enclosed cells changed, to 1.0; the number of cells written)."""
    occ = np.asarray(occ, dtype=np.float32)
    inside = enclosed(occ, unknown_is_filled, outside)
    out = occ.copy()
    out[inside] = np.float32(1.0)
    return out, int(inside.sum())


# ---- the cases the tests share ----
def _block(shape, free=()):
    occ = np.ones(shape, np.float32)
    for cell in free:
        occ[cell] = 0.0
    return occ


def hand_cases():
    """[(name, occupancy, unknown_is_filled, number of cells filled)], the counts derived by hand."""
    nan = np.float32(np.nan)
    known = {name: occ for name, occ, _ in T.known_answer_cases()}
    cases = []
    cases.append(("shell_3", _block((3, 3, 3), [(1, 1, 1)]), True, 1))
    cases.append(("shell_with_a_cavity", known["shell_with_a_cavity"], True, 27))            # the 3 x 3 x 3 cavity
    # the gap between the two shells (9^3 - 5^3) and the centre cell of the inner one
    cases.append(("nested_shells", known["nested_shells"], True, 9 ** 3 - 5 ** 3 + 1))
    cases.append(("two_cavities", known["two_cavities"], True, 2 * 3 * 2 * 3))
    # a corridor from the face x = 0 ends at (1, 1, 1); the cavity touches it across an edge / a vertex only
    cases.append(("contact_across_an_edge", _block((4, 4, 3), [(0, 1, 1), (1, 1, 1), (2, 2, 1)]), True, 1))
    cases.append(("contact_across_a_vertex", _block((4, 4, 4), [(0, 1, 1), (1, 1, 1), (2, 2, 2)]), True, 1))
    cases.append(("tunnel_to_a_face", _block((5, 5, 5), [(2, 2, 2), (2, 2, 3), (2, 2, 4)]), True, 0))
    # an unknown shell round a free cell in a free grid: a wall only when unknown counts as filled
    unknown_shell = np.zeros((5, 5, 5), np.float32)
    unknown_shell[1:4, 1:4, 1:4] = 0.5
    unknown_shell[2, 2, 2] = 0.0
    cases.append(("unknown_shell_filled", unknown_shell, True, 1))
    cases.append(("unknown_shell_passable", unknown_shell, False, 0))
    # an unknown cell inside a filled shell: filled already, or an enclosed passable cell
    unknown_cavity = _block((3, 3, 3))
    unknown_cavity[1, 1, 1] = 0.5
    cases.append(("unknown_cavity_filled", unknown_cavity, True, 0))
    cases.append(("unknown_cavity_passable", unknown_cavity, False, 1))
    # NaN is passable: in a wall's face centre it opens the cavity, in a corner it does not, in the cavity it is filled
    occ = _block((3, 3, 3), [(1, 1, 1)])
    occ[1, 1, 0] = nan
    cases.append(("nan_in_a_wall", occ, True, 0))
    occ = _block((3, 3, 3), [(1, 1, 1)])
    occ[0, 0, 0] = nan
    cases.append(("nan_in_a_corner", occ, True, 1))
    occ = _block((3, 3, 3))
    occ[1, 1, 1] = nan
    cases.append(("nan_in_the_cavity", occ, True, 1))
    # values that are filled or outside keep their bits: 0.7 walls, -0.0 outside, 0.3 inside
    occ = np.full((6, 5, 4), -0.0, np.float32)
    occ[1:5, 1:4, 1:3] = 0.7
    occ[2:4, 2, 1:3] = 0.3
    occ[2:4, 2, 0] = 0.7
    occ[2:4, 2, 3] = 0.7
    cases.append(("odd_values", occ, True, 4))
    return cases


def snake(shape, sealed=True):
    """One corridor that runs along every second Z line of a filled block and turns at alternating ends (the `_snake`
    of test_gpu_components.py), one cell away from every face of the grid so that walls seal it; sealed=False opens
    one border cell at its far end."""
    nx, ny, nz = shape
    occ = np.ones(shape, np.float32)
    lines = []
    for k, x in enumerate(range(1, nx - 1, 2)):
        ys = list(range(1, ny - 1, 2))
        lines += [(x, y) for y in (ys if k % 2 == 0 else ys[::-1])]
    for k, (x, y) in enumerate(lines):
        occ[x, y, 1:nz - 1] = 0.0
        if k + 1 < len(lines):
            x2, y2 = lines[k + 1]
            occ[(x + x2) // 2, (y + y2) // 2, nz - 2 if k % 2 == 0 else 1] = 0.0
    corridor = int((occ == 0.0).sum())
    if not sealed:
        x, y = lines[-1]
        occ[x, y, 0 if len(lines) % 2 == 0 else nz - 1] = 0.0
    return occ, corridor


def random_pockets(shape, p_filled, seed, sprinkle=False):
    """A random grid: filled with probability p_filled, free otherwise; sprinkle=True adds 2 % of 0.5 and 1 % of NaN."""
    rng = np.random.default_rng(seed)
    occ = (rng.random(shape) < p_filled).astype(np.float32)
    if sprinkle:
        u = rng.random(shape)
        occ[u < 0.02] = 0.5
        occ[u > 0.99] = np.nan
    return occ
