"""CPU restatement of vgt_hip_check_spheres (include/vgt_hip.h): a body of S spheres attached to L links, in B
configurations, against a signed distance field.  numpy float64 over the oracle's EstimateLocationDistance
(oracle.estimate_distance) and its coarse gradient with edge gradients (oracle.coarse_gradient(sdf, res, True)), gathered
at the cell of each centre as tests/projection_ref.py gathers them.

Not part of the oracle library (like tests/projection_ref.py).  Per (configuration b, sphere s), literally:

    w_r       = ((m[r]*x + m[4+r]*y) + m[8+r]*z) + m[12+r]     m = link_poses[b, sphere_link[s]], column-major
    d, has    = EstimateLocationDistance(w)                      (a link outside [0, L): no value, nothing is read)
    clearance = d - radius                                       NaN without a value
    gradient  = rotation * coarse gradient of w's cell           NaN x3 without a value

every operator a numpy temporary of its own, so nothing is fused.  Per configuration the reductions are done with masks:
num_outside = the spheres without a value; num_below = those with a value and clearance <= minimum_clearance;
min_clearance / min_sphere = the least non-NaN clearance among the spheres with a value and the FIRST index that has it
(NaN and -1 when there is none); min_gradient = that sphere's gradient; status by the three rules of the header.
"""
import collections

import numpy as np

CLEAR, COLLISION, NO_VALUE = 0, 1, 2

SphereChecks = collections.namedtuple(
    "SphereChecks", "status min_clearance min_sphere num_below num_outside min_gradient sphere_clearance sphere_gradient")


def _grid_frame(points, grid_from_world):
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    if grid_from_world is None:
        return x, y, z
    M = np.asarray(grid_from_world, dtype=np.float64).reshape(16)                   # column-major
    return (M[0] * x + M[4] * y + M[8] * z + M[12],
            M[1] * x + M[5] * y + M[9] * z + M[13],
            M[2] * x + M[6] * y + M[10] * z + M[14])


def world_centres(spheres_xyzr, sphere_link, link_poses):
    """-> (w [B, S, 3], link_ok [S]); rows of spheres whose link is out of range are NaN."""
    xyzr = np.asarray(spheres_xyzr, dtype=np.float64).reshape(-1, 4)
    link = np.asarray(sphere_link, dtype=np.int64).reshape(-1)
    poses = np.asarray(link_poses, dtype=np.float64)
    b, links = poses.shape[0], poses.shape[1]
    poses = poses.reshape(b, links, 16)
    link_ok = (link >= 0) & (link < links)
    w = np.full((b, len(xyzr), 3), np.nan)
    if not link_ok.any() or b == 0:
        return w, link_ok
    m = poses[:, link[link_ok], :]                                                  # [B, S', 16]
    x, y, z = xyzr[link_ok, 0], xyzr[link_ok, 1], xyzr[link_ok, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            a = m[:, :, r] * x
            t = m[:, :, 4 + r] * y
            a = a + t
            t = m[:, :, 8 + r] * z
            a = a + t
            w[:, link_ok, r] = a + m[:, :, 12 + r]
    return w, link_ok


def check_spheres(oracle, sdf, resolution, spheres_xyzr, sphere_link, link_poses, minimum_clearance=0.0,
                  outside_is_collision=False, grid_from_world=None, rotation=None):
    """-> SphereChecks, the per-sphere outputs always included"""
    field = np.ascontiguousarray(sdf, dtype=np.float32)
    resolution = float(resolution)
    xyzr = np.asarray(spheres_xyzr, dtype=np.float64).reshape(-1, 4)
    w, link_ok = world_centres(xyzr, sphere_link, link_poses)
    b, s = w.shape[0], w.shape[1]
    clearance = np.full((b, s), np.nan)
    gradient = np.full((b, s, 3), np.nan)
    has = np.zeros((b, s), dtype=bool)
    if b * s > 0 and field.size > 0:
        points = w.reshape(-1, 3)
        d, inside = oracle.estimate_distance(field, resolution, points, grid_from_world)
        inside = inside & np.repeat(link_ok[None, :], b, axis=0).reshape(-1)
        cell_gradient, _ = oracle.coarse_gradient(field, resolution, True)
        if rotation is not None:
            R = np.asarray(rotation, dtype=np.float64).reshape(9)                   # row-major
            gx, gy, gz = cell_gradient[..., 0], cell_gradient[..., 1], cell_gradient[..., 2]
            with np.errstate(invalid="ignore", over="ignore"):
                cell_gradient = np.stack([R[0] * gx + R[1] * gy + R[2] * gz,
                                          R[3] * gx + R[4] * gy + R[5] * gz,
                                          R[6] * gx + R[7] * gy + R[8] * gz], axis=-1)
        inv = 1.0 / resolution
        with np.errstate(invalid="ignore", over="ignore"):
            gfx, gfy, gfz = _grid_frame(points[inside], grid_from_world)
            ix = np.floor(gfx * inv).astype(np.int64)
            iy = np.floor(gfy * inv).astype(np.int64)
            iz = np.floor(gfz * inv).astype(np.int64)
            flat_clearance = np.full(b * s, np.nan)
            flat_clearance[inside] = d[inside] - np.tile(xyzr[:, 3], b)[inside]
        flat_gradient = np.full((b * s, 3), np.nan)
        flat_gradient[inside] = cell_gradient[ix, iy, iz]
        clearance = flat_clearance.reshape(b, s)
        gradient = flat_gradient.reshape(b, s, 3)
        has = inside.reshape(b, s)

    num_outside = np.sum(~has, axis=1).astype(np.int32)
    with np.errstate(invalid="ignore"):
        below = has & (clearance <= float(minimum_clearance))
    num_below = np.sum(below, axis=1).astype(np.int32)
    candidate = has & ~np.isnan(clearance)
    min_clearance = np.full(b, np.nan)
    min_sphere = np.full(b, -1, dtype=np.int32)
    min_gradient = np.full((b, 3), np.nan)
    for i in range(b):
        if not candidate[i].any():
            continue
        least = np.min(clearance[i][candidate[i]])
        first = int(np.flatnonzero(candidate[i] & (clearance[i] == least))[0])      # (-0.0 == 0.0: the first of them)
        min_clearance[i] = clearance[i, first]
        min_sphere[i] = first
        min_gradient[i] = gradient[i, first]
    collision = (num_below > 0) | (bool(outside_is_collision) & (num_outside > 0))
    status = np.where(collision, COLLISION, np.where(min_sphere != -1, CLEAR, NO_VALUE)).astype(np.uint8)
    return SphereChecks(status, min_clearance, min_sphere, num_below, num_outside, min_gradient, clearance, gradient)
