"""The tolerant checker of the nearest-other-class transform (contract: include/vgt_hip.h, vgt_hip_nearest_dev).  Plain
numpy.  The reference is the squared distance to the other class, from oracle.edt3d (run once with sites at the filled
cells and once at the free cells) or, for grids up to about 20^3, by brute force; `check` never compares indices, so
ties need no exemption: any cell of the other class at the minimal distance passes, every other answer fails."""
import numpy as np

NO_INDEX = -1
NO_DISTANCE = 0x7fffffff


def reference_d2(filled):
    """float64 squared distance of every cell to the nearest cell of the other class, inf where there is none."""
    from oracle import oracle as O
    filled = np.asarray(filled, dtype=bool)
    to_filled = O.edt3d(np.where(filled, 0.0, np.inf))
    to_free = O.edt3d(np.where(filled, np.inf, 0.0))
    return np.where(filled, to_free, to_filled)


def brute_force_d2(filled, chunk=512):
    """The same by comparing every cell with every cell of the other class, `chunk` query cells at a time."""
    filled = np.asarray(filled, dtype=bool)
    coords = np.stack(np.unravel_index(np.arange(filled.size), filled.shape), axis=1).astype(np.int64)
    flat = filled.ravel()
    out = np.full(filled.size, np.inf)
    for cls in (False, True):
        queries = np.flatnonzero(flat == cls)
        sites = coords[flat != cls]
        if sites.size == 0:
            continue
        for first in range(0, queries.size, chunk):
            q = queries[first:first + chunk]
            d = ((coords[q][:, None, :] - sites[None, :, :]) ** 2).sum(axis=2)
            out[q] = d.min(axis=1)
    return out.reshape(filled.shape)


def check(filled, nearest, d2=None, reference=None):
    """Asserts the contract for EVERY cell.  `reference`: reference_d2(filled), when the caller already has it."""
    filled = np.asarray(filled, dtype=bool)
    n = filled.size
    assert isinstance(nearest, np.ndarray) and nearest.dtype == np.int32, "nearest must be int32"
    assert nearest.size == n, "nearest must hold one entry per cell"
    ref = (reference_d2(filled) if reference is None else np.asarray(reference, dtype=np.float64)).ravel()
    got = nearest.ravel().astype(np.int64)
    flat = filled.ravel()
    none = np.isinf(ref)
    bad = np.flatnonzero((got == NO_INDEX) != none)
    assert bad.size == 0, "cell %d: nearest %d, reference d2 %r" % (bad[0], got[bad[0]], float(ref[bad[0]]))
    have = ~none
    cells = np.flatnonzero(have)
    target = got[have]
    bad = np.flatnonzero((target < 0) | (target >= n))
    assert bad.size == 0, "cell %d: nearest %d is outside the grid" % (cells[bad[0]], target[bad[0]])
    bad = np.flatnonzero(flat[target] == flat[have])
    assert bad.size == 0, "cell %d: nearest %d is of the cell's own class" % (cells[bad[0]], target[bad[0]])
    here = np.stack(np.unravel_index(cells, filled.shape), axis=1).astype(np.int64)
    there = np.stack(np.unravel_index(target, filled.shape), axis=1).astype(np.int64)
    dist = ((here - there) ** 2).sum(axis=1)
    bad = np.flatnonzero(dist != ref[have])
    assert bad.size == 0, "cell %d: nearest %d lies at d2 %d, the minimum is %r" % (
        cells[bad[0]], target[bad[0]], dist[bad[0]], float(ref[have][bad[0]]))
    if d2 is not None:
        assert isinstance(d2, np.ndarray) and d2.dtype == np.int32, "d2 must be int32"
        assert d2.size == n, "d2 must hold one entry per cell"
        want = np.where(none, float(NO_DISTANCE), ref)
        bad = np.flatnonzero(d2.ravel().astype(np.float64) != want)
        assert bad.size == 0, "cell %d: d2 %d, the minimum is %r" % (bad[0], d2.ravel()[bad[0]], float(want[bad[0]]))
