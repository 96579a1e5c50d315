"""CPU restatement of SignedDistanceField::ProjectLocationOutOfCollisionToMinimumDistance4d
(include/voxelized_geometry_tools/signed_distance_field.hpp:1111-1203) for a batch of points: numpy float64 over the
oracle's EstimateLocationDistance (oracle.estimate_distance) and its coarse gradient with edge gradients
(oracle.coarse_gradient(sdf, res, True)), the cell of a point found as floor(g * (1 / res)) like the estimate does.

Not part of the oracle library (like tests/mesh_ref.py).  The loop per point, literally:

    not in the grid                      -> the point, unchanged, with a value                       (OUTSIDE)
    margin   = minimum_distance + resolution * stepsize_multiplier * 1e-3
    max_step = resolution * stepsize_multiplier
    d        = EstimateLocationDistance(point)
    while d <= minimum_distance:
        g = rotation * coarse gradient of the point's cell;   no value, or |g| <= resolution * 0.25 -> nothing  (FLAT)
        point += g.normalized() * min(max_step, margin - d);  d = EstimateLocationDistance(point)
    -> the point                                                                                       (OK)

and the two things the reference leaves open, as include/vgt_hip.h closes them: after `max_iterations` steps with
d <= minimum_distance still -> ITERATION_LIMIT (0 selects ceil(2 * (nx + ny + nz) / stepsize_multiplier)); a step that
leaves the grid (the reference throws there) -> LEFT_GRID.  FLAT, LEFT_GRID and ITERATION_LIMIT have no value and a
NaN position.

The operation order of the step is the one include/vgt_hip.h pins, every operator a numpy temporary of its own, so
nothing is fused:  norm = sqrt((gx*gx + gy*gy) + gz*gz);  n_a = g_a / norm;  loc_a = loc_a + n_a * step.
"""
import math

import numpy as np

OK, OUTSIDE, FLAT_GRADIENT, LEFT_GRID, ITERATION_LIMIT = 0, 1, 2, 3, 4


def default_max_iterations(shape, stepsize_multiplier):
    nx, ny, nz = shape
    return min(int(math.ceil(2.0 * float(nx + ny + nz) / float(stepsize_multiplier))), 2 ** 31 - 1)


def _grid_frame(points, grid_from_world):
    x, y, z = points[:, 0], points[:, 1], points[:, 2]
    if grid_from_world is None:
        return x, y, z
    M = np.asarray(grid_from_world, dtype=np.float64).reshape(16)                   # column-major
    return (M[0] * x + M[4] * y + M[8] * z + M[12],
            M[1] * x + M[5] * y + M[9] * z + M[13],
            M[2] * x + M[6] * y + M[10] * z + M[14])


def project_out_of_collision(oracle, sdf, resolution, queries, minimum_distance=0.0, stepsize_multiplier=0.1,
                             max_iterations=0, grid_from_world=None, rotation=None):
    """-> (position [N, 3] float64, has_value [N] bool, status [N] uint8, iterations [N] int32)"""
    field = np.ascontiguousarray(sdf, dtype=np.float32)
    resolution = float(resolution)
    minimum_distance = float(minimum_distance)
    stepsize_multiplier = float(stepsize_multiplier)
    location = np.array(queries, dtype=np.float64).reshape(-1, 3)                   # (a copy: stepped in place)
    n = len(location)
    if max_iterations == 0:
        max_iterations = default_max_iterations(field.shape, stepsize_multiplier)
    gradient, gradient_has = oracle.coarse_gradient(field, resolution, True)
    if rotation is not None:
        R = np.asarray(rotation, dtype=np.float64).reshape(9)                       # row-major
        gx, gy, gz = gradient[..., 0], gradient[..., 1], gradient[..., 2]
        gradient = np.stack([R[0] * gx + R[1] * gy + R[2] * gz,
                             R[3] * gx + R[4] * gy + R[5] * gz,
                             R[6] * gx + R[7] * gy + R[8] * gz], axis=-1)
    margin = minimum_distance + resolution * stepsize_multiplier * 1e-3
    max_step = resolution * stepsize_multiplier
    inv = 1.0 / resolution

    status = np.full(n, OK, dtype=np.uint8)
    iterations = np.zeros(n, dtype=np.int32)
    d, inside = oracle.estimate_distance(field, resolution, location, grid_from_world)
    status[~inside] = OUTSIDE
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        live = np.flatnonzero(inside & (d <= minimum_distance))
        while len(live):
            at_limit = iterations[live] >= max_iterations
            status[live[at_limit]] = ITERATION_LIMIT
            live = live[~at_limit]
            if not len(live):
                break
            gfx, gfy, gfz = _grid_frame(location[live], grid_from_world)
            ix = np.floor(gfx * inv).astype(np.int64)
            iy = np.floor(gfy * inv).astype(np.int64)
            iz = np.floor(gfz * inv).astype(np.int64)
            g = gradient[ix, iy, iz]
            gx, gy, gz = g[:, 0], g[:, 1], g[:, 2]
            norm = np.sqrt((gx * gx + gy * gy) + gz * gz)
            flat = ~gradient_has[ix, iy, iz] | (norm <= resolution * 0.25)
            status[live[flat]] = FLAT_GRADIENT
            live, gx, gy, gz, norm = live[~flat], gx[~flat], gy[~flat], gz[~flat], norm[~flat]
            if not len(live):
                break
            to_margin = margin - d[live]
            step = np.where(to_margin < max_step, to_margin, max_step)              # std::min(max_step, margin - d)
            location[live, 0] = location[live, 0] + (gx / norm) * step
            location[live, 1] = location[live, 1] + (gy / norm) * step
            location[live, 2] = location[live, 2] + (gz / norm) * step
            iterations[live] += 1
            d[live], still_inside = oracle.estimate_distance(field, resolution, location[live], grid_from_world)
            status[live[~still_inside]] = LEFT_GRID
            live = live[still_inside]
            live = live[d[live] <= minimum_distance]
    has_value = (status == OK) | (status == OUTSIDE)
    location[~has_value] = np.nan
    return location, has_value, status, iterations
