"""numpy restatement of the four SDF consumers of csrc/cell_kernels.hip, written from the definitions in the reference's
signed_distance_field.hpp (line numbers below) and the operation order that cell_kernels.hip documents:

  coarse_gradient     GetGridAlignedIndexCoarseGradient (:922-1025) for every voxel, GetIndexCoarseGradient's rotation
                      (:903-920) on request
  estimate_distance   EstimateLocationDistance (:808-835 over :260-379)
  fine_gradient       GetLocationFineGradient (:1051-1092 over :214-255)
  local_extrema_map   ComputeLocalExtremaMap over FollowGradientsToLocalExtremaUnsafe (:382-480), GradientIsEffectiveFlat
                      (:482-497) and GetNextFromGradient (:499-538), walked literally, one start cell after the other

Everything is float64 element by element, one rounding per operation (numpy has no fused multiply-add), in the order
of the kernels, so the results are meant to be bit-identical to theirs.  Fields are float32 [nx, ny, nz]; the interior
coarse gradient takes its difference in float32 as the reference's expression does.  Returns follow the oracle:
(value, has_value[, window_too_large]).
"""
import numpy as np

NAN = float("nan")
STEP_FACTOR = 0.06125          # GradientIsEffectiveFlat / GetNextFromGradient: step_resolution = Resolution() * 0.06125


def _field(sdf):
    field = np.ascontiguousarray(sdf, dtype=np.float32)
    assert field.ndim == 3
    return field


def rotate(rotation, g):
    """OriginTransform() * gradient for [..., 3] gradients: rows of the 3x3 `rotation`, left to right."""
    if rotation is None:
        return g
    m = np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
    gx, gy, gz = g[..., 0], g[..., 1], g[..., 2]
    with np.errstate(all="ignore"):
        return np.stack([m[0] * gx + m[1] * gy + m[2] * gz,
                         m[3] * gx + m[4] * gy + m[5] * gz,
                         m[6] * gx + m[7] * gy + m[8] * gz], axis=-1)


def coarse_gradient(sdf, resolution, enable_edge_gradients=False, rotation=None):
    """-> (gradient [nx, ny, nz, 3] float64, has_value [nx, ny, nz] bool); NaN where there is no value."""
    field = _field(sdf)
    res = float(resolution)
    shape = field.shape
    idx = np.indices(shape)
    interior = np.ones(shape, dtype=bool)
    for a in range(3):
        interior &= (idx[a] > 0) & (idx[a] < shape[a] - 1)
    grad = np.zeros(shape + (3,), dtype=np.float64)
    inv_twice_resolution = 1.0 / (2.0 * res)
    with np.errstate(all="ignore"):
        for a in range(3):
            n = shape[a]
            low = np.maximum(idx[a] - 1, 0)
            high = np.minimum(idx[a] + 1, n - 1)
            lo_idx, hi_idx = list(idx), list(idx)
            lo_idx[a], hi_idx[a] = low, high
            lo_v, hi_v = field[tuple(lo_idx)], field[tuple(hi_idx)]
            # interior (:935-947): float difference, then the double product
            g_in = (hi_v - lo_v).astype(np.float64) * inv_twice_resolution
            # on a face (:956-1010): double difference times 1 / increment, 0 where the axis has no second cell
            increment = (high - low).astype(np.float64) * res
            positive = increment > 0.0
            inv_increment = np.where(positive, 1.0 / np.where(positive, increment, 1.0), 0.0)
            g_edge = np.where(positive, (hi_v.astype(np.float64) - lo_v.astype(np.float64)) * inv_increment, 0.0)
            grad[..., a] = np.where(interior, g_in, g_edge)
    has = interior | bool(enable_edge_gradients)
    has = np.broadcast_to(has, shape).copy()
    grad = rotate(rotation, grad)
    grad[~has] = NAN
    return grad, has


def _axis_interpolation_indices(initial, size, offset):
    """GetAxisInterpolationIndices (:278-312) on arrays."""
    up = offset >= 0.0                                         # false for NaN, like the reference's else branch
    # offset >= 0: (i, i + 1), or past the end (i - 1, i), or on a one-cell axis (i, i)
    up_over = initial + 1 >= size
    lower_up = np.where(up_over, np.where(initial - 1 < 0, initial, initial - 1), initial)
    upper_up = np.where(up_over, initial, initial + 1)
    # offset < 0: (i - 1, i), or before the start (i, i + 1), or on a one-cell axis (i, i)
    down_under = initial - 1 < 0
    lower_down = np.where(down_under, initial, initial - 1)
    upper_down = np.where(down_under, np.where(initial + 1 >= size, initial, initial + 1), initial)
    return np.where(up, lower_up, lower_down), np.where(up, upper_up, upper_down)


def _corrected_center_distance(field, x, y, z, res):
    """GetCorrectedCenterDistance (:260-275): `>= 0.0` sends +0.0 and -0.0 down, NaN up (it stays NaN)."""
    nominal = field[x, y, z].astype(np.float64)
    offset = res * 0.5
    with np.errstate(all="ignore"):
        return np.where(nominal >= 0.0, nominal - offset, nominal + offset)


def _lerp(a, b, t):
    with np.errstate(all="ignore"):
        return a * (1.0 - t) + b * t


def to_grid_frame(queries, grid_from_world=None):
    """M * (x, y, z, 1) for column-major M, row by row, left to right; the query itself when M is None."""
    q = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 3)
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    if grid_from_world is None:
        return x, y, z
    m = np.ascontiguousarray(grid_from_world, dtype=np.float64).reshape(16)
    with np.errstate(all="ignore"):
        return (m[0] * x + m[4] * y + m[8] * z + m[12],
                m[1] * x + m[5] * y + m[9] * z + m[13],
                m[2] * x + m[6] * y + m[10] * z + m[14])


def estimate_distance(sdf, resolution, queries, grid_from_world=None):
    """-> (distance [N] float64, has_value [N] bool); NaN where the location is not in the grid."""
    field = _field(sdf)
    res = float(resolution)
    nx, ny, nz = field.shape
    g = to_grid_frame(queries, grid_from_world)
    inv = 1.0 / res
    with np.errstate(all="ignore"):
        f = [np.floor(c * inv) for c in g]
        has = np.ones(len(g[0]), dtype=bool)
        for c, n in zip(f, (nx, ny, nz)):
            has &= (c >= 0.0) & (c < float(n))                  # also false for NaN
        out = np.full(len(has), NAN, dtype=np.float64)
        if not has.any():
            return out, has
        gx, gy, gz = (c[has] for c in g)
        ix, iy, iz = (c[has].astype(np.int64) for c in f)
        lower, upper, t = [], [], []
        for c, i, n in ((gx, ix, nx), (gy, iy, ny), (gz, iz, nz)):
            centre = (i.astype(np.float64) + 0.5) * res
            lo, hi = _axis_interpolation_indices(i, n, c - centre)
            low = (lo.astype(np.float64) + 0.5) * res
            lower.append(lo)
            upper.append(hi)
            t.append((c - low) / ((low + res) - low))
        (lx, ly, lz), (ux, uy, uz), (tx, ty, tz) = lower, upper, t
        mmm = _corrected_center_distance(field, lx, ly, lz, res)
        mmp = _corrected_center_distance(field, lx, ly, uz, res)
        mpm = _corrected_center_distance(field, lx, uy, lz, res)
        mpp = _corrected_center_distance(field, lx, uy, uz, res)
        pmm = _corrected_center_distance(field, ux, ly, lz, res)
        pmp = _corrected_center_distance(field, ux, ly, uz, res)
        ppm = _corrected_center_distance(field, ux, uy, lz, res)
        ppp = _corrected_center_distance(field, ux, uy, uz, res)
        mm, mp = _lerp(mmm, pmm, tx), _lerp(mmp, pmp, tx)
        pm, pp = _lerp(mpm, ppm, tx), _lerp(mpp, ppp, tx)
        lo, hi = _lerp(mm, pm, ty), _lerp(mp, pp, ty)
        out[has] = _lerp(lo, hi, tz)
    return out, has


BRANCH_BOTH, BRANCH_MINUS_ONLY, BRANCH_PLUS_ONLY, BRANCH_NONE = 0, 1, 2, 3


def fine_gradient_branches(sdf, resolution, queries, window, grid_from_world=None):
    """Which branch of ComputeAxisFineGradient every query takes on every axis: int [N, 3] of BRANCH_*, -1 where the
    query itself is not in the grid (the function is not reached)."""
    return _fine_gradient(sdf, resolution, queries, window, grid_from_world)[3]


def _fine_gradient(sdf, resolution, queries, window, grid_from_world):
    q = np.ascontiguousarray(queries, dtype=np.float64).reshape(-1, 3)
    w = abs(float(window))                                      # std::abs(nominal_window_size)
    point, point_ok = estimate_distance(sdf, resolution, q, grid_from_world)
    grad = np.full((len(q), 3), NAN, dtype=np.float64)
    branches = np.full((len(q), 3), -1, dtype=np.int64)
    with np.errstate(all="ignore"):
        for a in range(3):
            lo_q, hi_q = q.copy(), q.copy()
            lo_q[:, a] = q[:, a] - w                            # stepped in the frame of the query, before the transform
            hi_q[:, a] = q[:, a] + w
            minus, minus_ok = estimate_distance(sdf, resolution, lo_q, grid_from_world)
            plus, plus_ok = estimate_distance(sdf, resolution, hi_q, grid_from_world)
            both = (plus - minus) / (hi_q[:, a] - lo_q[:, a])
            minus_only = (point - minus) / (q[:, a] - lo_q[:, a])
            plus_only = (plus - point) / (hi_q[:, a] - q[:, a])
            branch = np.where(minus_ok & plus_ok, BRANCH_BOTH,
                              np.where(minus_ok, BRANCH_MINUS_ONLY, np.where(plus_ok, BRANCH_PLUS_ONLY, BRANCH_NONE)))
            grad[:, a] = np.choose(branch, [both, minus_only, plus_only, np.full(len(q), NAN)])
            branches[:, a] = np.where(point_ok, branch, -1)
    thrown = point_ok & (branches == BRANCH_NONE).any(axis=1)   # the reference throws "Window size ... too large"
    has = point_ok & ~thrown
    grad[~has] = NAN
    return grad, has, bool(thrown.any()), branches


def fine_gradient(sdf, resolution, queries, window, grid_from_world=None):
    """-> (gradient [N, 3] float64, has_value [N] bool, window_too_large); NaN where there is no value."""
    return _fine_gradient(sdf, resolution, queries, window, grid_from_world)[:3]


def successors(sdf, resolution, rotation=None):
    """Per cell (flat index, X-major): (flat [cells] bool, next [cells] int64, -1 = off the grid).  `next` of a cell that
    is not flat and moves nowhere (a NaN component and none beyond the threshold) is the cell itself."""
    field = _field(sdf)
    res = float(resolution)
    shape = field.shape
    grad, _ = coarse_gradient(field, res, True, rotation)
    step = res * STEP_FACTOR
    with np.errstate(all="ignore"):
        flat = (np.abs(grad) <= step).all(axis=-1)
        working = np.where((field < np.float32(0.0))[..., None], grad * -1.0, grad)
        move = np.where(working > step, 1, np.where(working < -step, -1, 0))
    target = np.indices(shape).transpose(1, 2, 3, 0) + move
    inside = ((target >= 0) & (target < np.array(shape))).all(axis=-1)
    nxt = (target[..., 0] * shape[1] + target[..., 1]) * shape[2] + target[..., 2]
    return flat.reshape(-1), np.where(inside, nxt, -1).reshape(-1)


def local_extrema_map(sdf, resolution, rotation=None):
    """-> [nx, ny, nz, 3] float64: the walk of FollowGradientsToLocalExtremaUnsafe from every cell in X-major order."""
    field = _field(sdf)
    res = float(resolution)
    nx, ny, nz = field.shape
    flat, nxt = successors(field, res, rotation)
    flat, nxt = flat.tolist(), nxt.tolist()
    total = nx * ny * nz
    neg_inf, inf = float("-inf"), float("inf")

    def location(cell):                                          # GridIndexToLocationInGridFrame: the cell centre
        return ((float(cell // (ny * nz)) + 0.5) * res, (float((cell // nz) % ny) + 0.5) * res,
                (float(cell % nz) + 0.5) * res)

    def is_stored(v):
        return v[0] != neg_inf and v[1] != neg_inf and v[2] != neg_inf

    stored = [(neg_inf, neg_inf, neg_inf)] * total
    for start in range(total):
        if is_stored(stored[start]):
            continue
        if flat[start]:
            stored[start] = location(start)
            continue
        path = {start: 1}
        current = start
        while True:
            current = nxt[current]
            if path.get(current, 0) != 0:                        # been here on this walk
                extremum = location(current)
                break
            if current < 0:                                      # pushed past the edge
                extremum = (inf, inf, inf)
                break
            path[current] = 1
            if is_stored(stored[current]):
                extremum = stored[current]
                break
            if flat[current]:
                extremum = location(current)
                break
        for cell in path:
            stored[cell] = extremum
    return np.array(stored, dtype=np.float64).reshape(nx, ny, nz, 3)
