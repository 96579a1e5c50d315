"""CPU restatement of the reference's mesh rasterizer (src/voxelized_geometry_tools/mesh_rasterizer.cpp), numpy float64,
written after that file line by line (citations as mesh_rasterizer.cpp:LINE) and vectorised over candidate cells.

Every dot and cross product is written out as elementwise products and left-to-right sums -- numpy evaluates each
operator into a temporary of its own, so nothing is fused; np.dot / np.cross / einsum / @ are NOT used: their SIMD and
BLAS loops may fuse multiply-adds.  This is the operation order of csrc/mesh_kernels.hip (see its header comment).

Two closest-point rules:
  rule 0 (REFERENCE)  the literal port: the three edge candidates are ranked by their OWN squared norm (:82-84), i.e. by
                      their distance to the frame's origin, not to the query point
  rule 1 (NEAREST)    the same structure, the candidates ranked by their squared distance to the query point

Fixed where the reference calls into common_robotics_utilities (source not available): ClampValue = min/max;
VectorRejection(n, v) = v - ((n.v) / (n.n)) * n.  A triangle whose normal has squared norm 0, a non-finite vertex or an
index out of range raise ValueError (the device reports them as errors; the reference's behaviour there is unknown).
"""
import math

import numpy as np

RULE_REFERENCE = 0
RULE_NEAREST = 1
NOT_CONTAINED = "Triangle is not contained by occupancy map"          # :194-195
_CHUNK_CELLS = 1 << 21


def max_check_radius_squared(resolution):
    """:117-119"""
    min_check_radius = float(resolution) * 0.5
    max_check_radius = min_check_radius * math.sqrt(3.0)
    return math.pow(max_check_radius, 2.0)


def mesh_grid_for(vertices, resolution):
    """RasterizeMeshIntoOccupancyMapImpl, :243-269: ((nx, ny, nz), origin xyz) of the map the reference builds."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 3)
    resolution = float(resolution)
    if not (resolution > 0.0 and math.isfinite(resolution)):
        raise ValueError("resolution must be greater than zero")                     # :238-241
    if len(v) == 0 or not np.isfinite(v).all():
        raise ValueError("vertices must be finite and at least one")
    lower = [float(v[:, a].min()) for a in range(3)]                                 # :243-253
    upper = [float(v[:, a].max()) for a in range(3)]
    buffer_size = resolution * 2.0                                                   # :257
    counts = []
    for a in range(3):
        object_size = upper[a] - lower[a]                                            # :255
        grid_dimension = object_size + buffer_size                                   # :258-261
        counts.append(int(math.ceil(grid_dimension / resolution)))                   # VoxelGridSizes::FromGridSizes
    origin = np.array([lower[a] - resolution for a in range(3)], dtype=np.float64)   # :266-269
    return tuple(counts), origin


def _apply(m, x, y, z):
    """4x4 column-major transform, row by row, left to right."""
    return (m[0] * x + m[4] * y + m[8] * z + m[12],
            m[1] * x + m[5] * y + m[9] * z + m[13],
            m[2] * x + m[6] * y + m[10] * z + m[14])


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _same_side(pa, pb, p1, p2):
    """:30-38"""
    v_ab = _sub(pb, pa)
    cross1 = _cross(v_ab, _sub(p1, pa))
    cross2 = _cross(v_ab, _sub(p2, pa))
    return _dot(cross1, cross2) >= 0.0


def _closest_on_segment(pa, pb, q):
    """:45-57"""
    v_ab = _sub(pb, pa)
    v_aq = _sub(q, pa)
    ratio = _dot(v_ab, v_aq) / _dot(v_ab, v_ab)
    clamped = np.minimum(np.maximum(ratio, 0.0), 1.0)
    return (pa[0] + v_ab[0] * clamped, pa[1] + v_ab[1] * clamped, pa[2] + v_ab[2] * clamped)


def closest_point_on_triangle(v1, v2, v3, normal, q, rule):
    """CalcClosestPointOnTriangle, :59-102.  Every argument a triple of equally shaped float64 arrays."""
    inside = _same_side(v1, v2, v3, q) & _same_side(v2, v3, v1, q) & _same_side(v3, v1, v2, q)     # :40-42
    v_v1q = _sub(q, v1)                                                                             # :68
    b2 = _dot(normal, normal)
    scale = _dot(normal, v_v1q) / b2                                                                # VectorRejection
    projected = tuple(v1[a] + (v_v1q[a] - scale * normal[a]) for a in range(3))                     # :70-71
    c12 = _closest_on_segment(v1, v2, q)                                                            # :76-81
    c23 = _closest_on_segment(v2, v3, q)
    c31 = _closest_on_segment(v3, v1, q)
    if rule == RULE_REFERENCE:
        d12, d23, d31 = _dot(c12, c12), _dot(c23, c23), _dot(c31, c31)                              # :82-84
    elif rule == RULE_NEAREST:
        e12, e23, e31 = _sub(c12, q), _sub(c23, q), _sub(c31, q)
        d12, d23, d31 = _dot(e12, e12), _dot(e23, e23), _dot(e31, e31)
    else:
        raise ValueError("rule must be 0 or 1")
    first = (d12 <= d23) & (d12 <= d31)                                                             # :85-86
    second = (d23 <= d12) & (d23 <= d31)                                                            # :90-91
    edge = tuple(np.where(first, c12[a], np.where(second, c23[a], c31[a])) for a in range(3))
    return tuple(np.where(inside, projected[a], edge[a]) for a in range(3))


def _floor_index(g, inv):
    f = np.floor(g * inv)
    return np.clip(f, -2.0 ** 61, 2.0 ** 61).astype(np.int64)


def candidates(vertices, triangles, shape, resolution, world_from_grid=None, grid_from_world=None, enforce=False,
               rule=RULE_REFERENCE):
    """Yields (triangle, ix, iy, iz, distance_squared) arrays over every candidate cell, in chunks, triangle by
    triangle in ascending order.  enforce=False clamps the ranges to the grid first (outside cells are skipped by the
    reference anyway, :187-191)."""
    v = np.ascontiguousarray(vertices, dtype=np.float64).reshape(-1, 3)
    tri = np.ascontiguousarray(triangles, dtype=np.int64).reshape(-1, 3)
    if (world_from_grid is None) != (grid_from_world is None):
        raise ValueError("both transforms or neither")
    wfg = None if world_from_grid is None else np.asarray(world_from_grid, dtype=np.float64).reshape(16)
    gfw = None if grid_from_world is None else np.asarray(grid_from_world, dtype=np.float64).reshape(16)
    resolution = float(resolution)
    inv = 1.0 / resolution
    if len(tri) == 0:
        return
    if (tri < 0).any() or (tri >= len(v)).any():
        raise ValueError("triangle index out of range")                                   # vertices.at(), :122-124
    p = [tuple(v[tri[:, k], a] for a in range(3)) for k in range(3)]
    if not all(np.isfinite(c).all() for pk in p for c in pk):
        raise ValueError("non-finite vertex")
    v1v2 = _sub(p[1], p[0])                                                               # :126-127
    v1v3 = _sub(p[2], p[0])
    normal = _cross(v1v2, v1v3)                                                           # :131
    if not (_dot(normal, normal) > 0.0).all():
        raise ValueError("degenerate triangle")
    lo_xyz = tuple(np.minimum(np.minimum(p[0][a], p[1][a]), p[2][a]) for a in range(3))   # :133-139
    hi_xyz = tuple(np.maximum(np.maximum(p[0][a], p[1][a]), p[2][a]) for a in range(3))
    if gfw is not None:                                                                   # LocationToGridIndex, :141-144
        lo_g, hi_g = _apply(gfw, *lo_xyz), _apply(gfw, *hi_xyz)
    else:
        lo_g, hi_g = lo_xyz, hi_xyz
    lo = [_floor_index(lo_g[a], inv) for a in range(3)]
    hi = [_floor_index(hi_g[a], inv) for a in range(3)]
    if not enforce:
        for a in range(3):
            lo[a] = np.maximum(lo[a], 0)
            hi[a] = np.minimum(hi[a], shape[a] - 1)
    ext = [np.maximum(hi[a] - lo[a] + 1, 0) for a in range(3)]                            # :146-153 (empty when lo > hi)
    cells = ext[0] * ext[1] * ext[2]
    start = 0
    while start < len(tri):
        stop = start + 1
        total = int(cells[start])
        while stop < len(tri) and total + int(cells[stop]) <= _CHUNK_CELLS:
            total += int(cells[stop])
            stop += 1
        if total > 0:
            sl = slice(start, stop)
            t = np.repeat(np.arange(start, stop), cells[sl])
            first = np.cumsum(cells[sl]) - cells[sl]
            k = np.arange(total) - np.repeat(first, cells[sl])
            ey, ez = ext[1][t], ext[2][t]
            ix = lo[0][t] + k // (ey * ez)
            iy = lo[1][t] + (k // ez) % ey
            iz = lo[2][t] + k % ez
            cx = (ix.astype(np.float64) + 0.5) * resolution                               # GridIndexToLocation, :157-159
            cy = (iy.astype(np.float64) + 0.5) * resolution
            cz = (iz.astype(np.float64) + 0.5) * resolution
            q = _apply(wfg, cx, cy, cz) if wfg is not None else (cx, cy, cz)
            tv = [tuple(c[t] for c in pk) for pk in p]
            tn = tuple(c[t] for c in normal)
            closest = closest_point_on_triangle(tv[0], tv[1], tv[2], tn, q, rule)         # :161-162
            diff = _sub(closest, q)
            yield t, ix, iy, iz, _dot(diff, diff)                                         # :164
        start = stop


def rasterize(vertices, triangles, occupancy, resolution, world_from_grid=None, grid_from_world=None, enforce=False,
              rule=RULE_REFERENCE):
    """RasterizeMeshImpl into a copy of `occupancy` (float32 (nx, ny, nz)): intersecting cells are set to 1.0f, nothing
    else is touched.  enforce=True raises RuntimeError(NOT_CONTAINED) when an intersecting cell lies outside."""
    out = np.array(occupancy, dtype=np.float32, copy=True)
    nx, ny, nz = out.shape
    r2 = max_check_radius_squared(resolution)
    for _, ix, iy, iz, d2 in candidates(vertices, triangles, out.shape, resolution, world_from_grid, grid_from_world,
                                        enforce, rule):
        hit = d2 <= r2                                                                    # :182-183
        inside = (ix >= 0) & (ix < nx) & (iy >= 0) & (iy < ny) & (iz >= 0) & (iz < nz)
        if enforce and (hit & ~inside).any():
            raise RuntimeError(NOT_CONTAINED)                                             # :192-196
        sel = hit & inside
        out[ix[sel], iy[sel], iz[sel]] = np.float32(1.0)                                  # :187-191
    return out


def rasterize_into_new_map(vertices, triangles, resolution, rule=RULE_REFERENCE):
    """RasterizeMeshIntoOccupancyMap, :231-278: (occupancy, origin xyz); the map's transform is a pure translation."""
    shape, origin = mesh_grid_for(vertices, resolution)
    wfg = np.eye(4)
    wfg[:3, 3] = origin
    gfw = np.eye(4)
    gfw[:3, 3] = -origin                       # (the inverse of a pure translation, exactly)
    occ = rasterize(vertices, triangles, np.zeros(shape, np.float32), resolution, wfg.T.reshape(16), gfw.T.reshape(16),
                    True, rule)
    return occ, origin


def point_triangle_distance_squared(a, b, c, q):
    """Independent yardstick for rule 1: the barycentric-region closest point of a triangle (Ericson, Real-Time
    Collision Detection, 5.1.5), derived separately from the code above.  Triples of float64 arrays."""
    ab, ac, ap = _sub(b, a), _sub(c, a), _sub(q, a)
    d1, d2 = _dot(ab, ap), _dot(ac, ap)
    bp = _sub(q, b)
    d3, d4 = _dot(ab, bp), _dot(ac, bp)
    cp = _sub(q, c)
    d5, d6 = _dot(ab, cp), _dot(ac, cp)
    vc = d1 * d4 - d3 * d2
    vb = d5 * d2 - d1 * d6
    va = d3 * d6 - d5 * d4
    with np.errstate(divide="ignore", invalid="ignore"):
        t_ab = d1 / (d1 - d3)
        t_ac = d2 / (d2 - d6)
        t_bc = (d4 - d3) / ((d4 - d3) + (d5 - d6))
        denom = 1.0 / (va + vb + vc)
    vv, ww = vb * denom, vc * denom
    regions = [
        ((d1 <= 0.0) & (d2 <= 0.0), a),
        ((d3 >= 0.0) & (d4 <= d3), b),
        ((vc <= 0.0) & (d1 >= 0.0) & (d3 <= 0.0), tuple(a[k] + t_ab * ab[k] for k in range(3))),
        ((d6 >= 0.0) & (d5 <= d6), c),
        ((vb <= 0.0) & (d2 >= 0.0) & (d6 <= 0.0), tuple(a[k] + t_ac * ac[k] for k in range(3))),
        ((va <= 0.0) & ((d4 - d3) >= 0.0) & ((d5 - d6) >= 0.0), tuple(b[k] + t_bc * (c[k] - b[k]) for k in range(3))),
    ]
    closest = tuple(a[k] + ab[k] * vv + ac[k] * ww for k in range(3))
    for cond, point in reversed(regions):
        closest = tuple(np.where(cond, point[k], closest[k]) for k in range(3))
    diff = _sub(closest, q)
    return _dot(diff, diff)
