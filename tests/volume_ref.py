"""CPU restatement of vgt_hip_rasterize_spheres and vgt_hip_spheres_cover_points (include/vgt_hip.h): which cells of a
grid, or which points of a cloud, the spheres of B configurations of a sphere model cover, and the least configuration
(and sphere) that does.  numpy float64, brute force on purpose: every cell, or every point, against every sphere, by the
literal expressions of the header, every operator a numpy temporary of its own so that nothing is fused.  There is no
box and no pruning here, so it is independent of what the kernels skip.

    w_r    = ((m[r]*x + m[4+r]*y) + m[8+r]*z) + m[12+r]         m = link_poses[b, sphere_link[s]], column-major
    R      = radius + padding
    usable = link in [0, L), w finite, R finite and >= 0 (grid form: c finite too); not usable covers nothing
    covers = ((dx*dx + dy*dy) + dz*dz) <= R*R,  d_a = q_a - c_a

Grid form: c_a = M[a]*w0 + M[4+a]*w1 + M[8+a]*w2 + M[12+a] left to right (c = w without a transform), q_a = (i_a + 0.5) *
resolution; first_configuration[cell] = base + the least covering b, -1 without one; with `into` the unsigned minimum of
what it held and what is found.  Point form: q_r = ((T[r]*px + T[4+r]*py) + T[8+r]*pz) + T[12+r] on the float32
coordinates widened to double, c = w; a point with a non-finite coordinate or q is covered by nothing.
"""
import collections

import numpy as np

import body_ref

PointCover = collections.namedtuple("PointCover", "first_configuration first_sphere filtered")


def usable_spheres(spheres_xyzr, sphere_link, link_poses, padding, grid_from_world=None):
    """-> (c [B, S, 3] centres (in the grid frame with grid_from_world), R [S], usable [B, S])"""
    xyzr = np.asarray(spheres_xyzr, dtype=np.float64).reshape(-1, 4)
    w, link_ok = body_ref.world_centres(xyzr, sphere_link, link_poses)            # (the same w_r, operator by operator)
    with np.errstate(invalid="ignore", over="ignore"):
        R = xyzr[:, 3] + np.float64(padding)
        usable = link_ok[None, :] & np.isfinite(w).all(axis=2) & (np.isfinite(R) & (R >= 0.0))[None, :]
        c = w
        if grid_from_world is not None:
            M = np.asarray(grid_from_world, dtype=np.float64).reshape(16)
            c = np.empty_like(w)
            for a in range(3):
                t = M[a] * w[..., 0]
                u = M[4 + a] * w[..., 1]
                t = t + u
                u = M[8 + a] * w[..., 2]
                t = t + u
                c[..., a] = t + M[12 + a]
            usable = usable & np.isfinite(c).all(axis=2)
    return c, R, usable


def _covers(q, c, R):
    """q [..., 3] against one centre c [3] and R"""
    with np.errstate(invalid="ignore", over="ignore"):
        dx = q[..., 0] - c[0]
        dy = q[..., 1] - c[1]
        dz = q[..., 2] - c[2]
        xx = dx * dx
        yy = dy * dy
        zz = dz * dz
        return ((xx + yy) + zz) <= R * R


def cell_centre_axes(shape, resolution):
    """per axis: q_a = (i_a + 0.5) * resolution"""
    return [(np.arange(n, dtype=np.float64) + 0.5) * np.float64(resolution) for n in shape]


def cell_centres(shape, resolution):
    """[nx, ny, nz, 3]"""
    return np.stack(np.meshgrid(*cell_centre_axes(shape, resolution), indexing="ij"), axis=-1)


def _covers_cells(axes, c, R):
    """Every cell against one centre: the same operations per cell as _covers -- d_a * d_a depends on i_a alone, so each
    square is computed once per index of its axis and not once per cell; the two sums and the comparison are per cell."""
    with np.errstate(invalid="ignore", over="ignore"):
        dx = axes[0] - c[0]
        dy = axes[1] - c[1]
        dz = axes[2] - c[2]
        xx = dx * dx
        yy = dy * dy
        zz = dz * dz
        return ((xx[:, None, None] + yy[None, :, None]) + zz[None, None, :]) <= R * R


def rasterize_spheres(shape, resolution, spheres_xyzr, sphere_link, link_poses, padding=0.0, base=0, into=None,
                      grid_from_world=None):
    """-> first_configuration int32 of `shape`"""
    shape = tuple(int(n) for n in shape)
    c, R, usable = usable_spheres(spheres_xyzr, sphere_link, link_poses, padding, grid_from_world)
    found = np.full(shape, 0xffffffff, dtype=np.uint32) if into is None else np.array(into, dtype=np.int32).view(np.uint32)
    if found.size:
        axes = cell_centre_axes(shape, resolution)
        for b in range(c.shape[0]):
            covered = np.zeros(shape, dtype=bool)
            for s in np.flatnonzero(usable[b]):
                covered |= _covers_cells(axes, c[b, s], R[s])
            found[covered] = np.minimum(found[covered], np.uint32(base + b))
    return found.view(np.int32).reshape(shape)


def spheres_cover_points(points, spheres_xyzr, sphere_link, link_poses, padding=0.0, world_from_points=None):
    """-> PointCover (filtered always included)"""
    pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
    p = pts.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        q = p
        if world_from_points is not None:
            T = np.asarray(world_from_points, dtype=np.float64).reshape(16)
            q = np.empty_like(p)
            for r in range(3):
                t = T[r] * p[:, 0]
                u = T[4 + r] * p[:, 1]
                t = t + u
                u = T[8 + r] * p[:, 2]
                t = t + u
                q[:, r] = t + T[12 + r]
    ok = np.isfinite(p).all(axis=1) & np.isfinite(q).all(axis=1)
    c, R, usable = usable_spheres(spheres_xyzr, sphere_link, link_poses, padding)
    n = len(pts)
    first_b = np.full(n, -1, dtype=np.int32)
    first_s = np.full(n, -1, dtype=np.int32)
    for b in range(c.shape[0]):
        for s in np.flatnonzero(usable[b]):
            hit = ok & (first_b < 0) & _covers(q, c[b, s], R[s])
            first_b[hit] = b
            first_s[hit] = s
    filtered = pts.copy()
    filtered[first_b >= 0] = np.float32(np.nan)
    return PointCover(first_b, first_s, filtered)
