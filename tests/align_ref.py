"""CPU restatement of vgt_hip_align_points (include/vgt_hip.h): a point cloud under B pose hypotheses against a signed
distance field -- evaluate, tree_sum, solve, update and the loop (align) -- in numpy float64, every operator a temporary
of its own so that nothing is fused, in the order the header gives.  Not part of the oracle library (like
tests/body_ref.py); the estimate's three steps are restated here too, because the gradient needs its corners, and
tests/test_align_ref.py checks them against oracle.estimate_distance bit for bit.
"""
import collections

import numpy as np

CONVERGED, ITERATION_LIMIT, DEGENERATE, TOO_FEW = 0, 1, 2, 3

CloudAlignment = collections.namedtuple(
    "CloudAlignment", "poses status num_used num_outside num_rejected sum_squared evaluations normal_equations last_step")

# one pose's evaluation: sums [28] (H's 21 entries row-major over j <= k, b, e), the three counts, and per point the
# estimate, the gradient, the used mask and the 28 terms
Evaluation = collections.namedtuple("Evaluation", "sums num_used num_outside num_rejected d gradient used terms")


def tree_sum(values):
    """The one summation tree, along axis 0: groups of 64 consecutive entries (the last padded with +0.0), each reduced by
    v[i] = v[i] + v[i + h] for h = 32 ... 1; again on the group sums while more than one is left."""
    v = np.array(values, dtype=np.float64)
    while True:
        groups = (len(v) + 63) // 64
        padded = np.zeros((groups * 64,) + v.shape[1:], dtype=np.float64)
        padded[:len(v)] = v
        w = padded.reshape((groups, 64) + v.shape[1:])
        h = 32
        with np.errstate(invalid="ignore", over="ignore"):
            while h >= 1:
                w[:, :h] = w[:, :h] + w[:, h:2 * h]
                h //= 2
        v = w[:, 0].copy()
        if len(v) == 1:
            return v[0]


def _axis_indices(initial, size, offset):
    """GetAxisInterpolationIndices -> (lower, upper)"""
    up, down = initial + 1, initial - 1
    over, under = up >= size, down < 0
    lower_pos = np.where(over, np.where(under, initial, down), initial)
    upper_pos = np.where(over, initial, up)
    lower_neg = np.where(under, initial, down)
    upper_neg = np.where(under, np.where(over, initial, up), initial)
    positive = offset >= 0.0
    return np.where(positive, lower_pos, lower_neg), np.where(positive, upper_pos, upper_neg)


def _lerp(a, b, t):
    one_minus = 1.0 - t
    left = a * one_minus
    right = b * t
    return left + right


def world_points(points, pose):
    """w [N, 3] for float32 points [N, 3] and a column-major pose [16]"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3).astype(np.float64)
    m = np.asarray(pose, dtype=np.float64).reshape(16)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    w = np.empty_like(p)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(3):
            a = m[r] * x
            t = m[4 + r] * y
            a = a + t
            t = m[8 + r] * z
            a = a + t
            w[:, r] = a + m[12 + r]
    return w


def estimate_with_gradient(sdf, resolution, w, grid_from_world=None, rotation=None):
    """The estimate and the gradient of its interpolant at world locations w [N, 3] -> (d [N], g [N, 3], has [N]);
    d and g are NaN without a value."""
    field = np.ascontiguousarray(sdf, dtype=np.float32)
    nx, ny, nz = field.shape
    res = float(resolution)
    n = len(w)
    d = np.full(n, np.nan)
    g = np.full((n, 3), np.nan)
    x, y, z = w[:, 0], w[:, 1], w[:, 2]
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if grid_from_world is None:
            gx_, gy_, gz_ = x, y, z
        else:
            M = np.asarray(grid_from_world, dtype=np.float64).reshape(16)
            gx_ = M[0] * x + M[4] * y + M[8] * z + M[12]
            gy_ = M[1] * x + M[5] * y + M[9] * z + M[13]
            gz_ = M[2] * x + M[6] * y + M[10] * z + M[14]
        inv = 1.0 / res
        fx, fy, fz = np.floor(gx_ * inv), np.floor(gy_ * inv), np.floor(gz_ * inv)
        has = (fx >= 0.0) & (fx < nx) & (fy >= 0.0) & (fy < ny) & (fz >= 0.0) & (fz < nz)
        if not has.any():
            return d, g, has
        loc = [gx_[has], gy_[has], gz_[has]]
        cell = [fx[has].astype(np.int64), fy[has].astype(np.int64), fz[has].astype(np.int64)]
        lower, upper, t, span = [], [], [], []
        for axis, size in enumerate((nx, ny, nz)):
            centre = (cell[axis].astype(np.float64) + 0.5) * res
            lo, hi = _axis_indices(cell[axis], size, loc[axis] - centre)
            low = (lo.astype(np.float64) + 0.5) * res
            e = (low + res) - low
            lower.append(lo)
            upper.append(hi)
            span.append(e)
            t.append((loc[axis] - low) / e)

        def corner(a, b, c):
            nominal = field[a, b, c].astype(np.float64)
            offset = res * 0.5
            return np.where(nominal >= 0.0, nominal - offset, nominal + offset)

        (lx, ly, lz), (ux, uy, uz) = lower, upper
        mmm, mmp, mpm, mpp = corner(lx, ly, lz), corner(lx, ly, uz), corner(lx, uy, lz), corner(lx, uy, uz)
        pmm, pmp, ppm, ppp = corner(ux, ly, lz), corner(ux, ly, uz), corner(ux, uy, lz), corner(ux, uy, uz)
        tx, ty, tz = t
        mm, mp, pm, pp = _lerp(mmm, pmm, tx), _lerp(mmp, pmp, tx), _lerp(mpm, ppm, tx), _lerp(mpp, ppp, tx)
        d[has] = _lerp(_lerp(mm, pm, ty), _lerp(mp, pp, ty), tz)
        gx = _lerp(_lerp(pmm - mmm, ppm - mpm, ty), _lerp(pmp - mmp, ppp - mpp, ty), tz) / span[0]
        gy = _lerp(_lerp(mpm - mmm, ppm - pmm, tx), _lerp(mpp - mmp, ppp - pmp, tx), tz) / span[1]
        gz = _lerp(_lerp(mmp - mmm, pmp - pmm, tx), _lerp(mpp - mpm, ppp - ppm, tx), ty) / span[2]
        if rotation is not None:
            R = np.asarray(rotation, dtype=np.float64).reshape(9)                   # row-major
            gx, gy, gz = (R[0] * gx + R[1] * gy + R[2] * gz, R[3] * gx + R[4] * gy + R[5] * gz,
                          R[6] * gx + R[7] * gy + R[8] * gz)
        g[has] = np.stack([gx, gy, gz], axis=1)
    return d, g, has


def evaluate(sdf, resolution, points, pose, target_distance=0.0, max_residual=np.inf, pivot=None, grid_from_world=None,
             rotation=None):
    """One pose -> Evaluation"""
    p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
    n = len(p)
    finite_point = np.isfinite(p).all(axis=1)
    w = world_points(p, pose)
    d, g, has = estimate_with_gradient(sdf, resolution, w, grid_from_world, rotation)
    has = has & finite_point
    about = np.zeros(3) if pivot is None else np.asarray(pivot, dtype=np.float64).reshape(3)
    terms = np.zeros((n, 28))
    with np.errstate(invalid="ignore", over="ignore"):
        r = d - float(target_distance)
        used = has & np.isfinite(r) & np.isfinite(g).all(axis=1) & (np.abs(r) <= float(max_residual))
        q = w[used] - about
        gx, gy, gz, ru = g[used, 0], g[used, 1], g[used, 2], r[used]
        J = [gx, gy, gz,
             q[:, 1] * gz - q[:, 2] * gy,
             q[:, 2] * gx - q[:, 0] * gz,
             q[:, 0] * gy - q[:, 1] * gx]
        t = 0
        for j in range(6):
            for k in range(j, 6):
                terms[used, t] = J[j] * J[k]
                t += 1
        for j in range(6):
            terms[used, 21 + j] = J[j] * ru
        terms[used, 27] = ru * ru
    sums = tree_sum(terms)
    return Evaluation(sums, int(used.sum()), int((finite_point & ~has).sum()), int((has & ~used).sum()), d, g, used,
                      terms)


def solve(sums, damping):
    """The damped normal equations of sums[:27] -> delta [6], or None when degenerate."""
    f = np.float64
    A = [[f(0.0)] * 6 for _ in range(6)]
    t = 0
    for j in range(6):
        for k in range(j, 6):
            A[j][k] = A[k][j] = f(sums[t])
            t += 1
    b = [f(sums[21 + j]) for j in range(6)]
    scale = f(1.0) + f(damping)
    for j in range(6):
        A[j][j] = A[j][j] * scale
    L = [[f(0.0)] * 6 for _ in range(6)]
    D = [f(0.0)] * 6
    degenerate = False
    with np.errstate(all="ignore"):
        for j in range(6):
            d = A[j][j]
            for k in range(j):
                d = d - (L[j][k] * L[j][k]) * D[k]
            D[j] = d
            if not d > 0.0:
                degenerate = True
            for i in range(j + 1, 6):
                l = A[i][j]
                for k in range(j):
                    l = l - (L[i][k] * L[j][k]) * D[k]
                L[i][j] = l / d
        y = [f(0.0)] * 6
        for i in range(6):
            v = b[i]
            for k in range(i):
                v = v - L[i][k] * y[k]
            y[i] = v
        x = [f(0.0)] * 6
        for i in range(5, -1, -1):
            v = y[i] / D[i]
            for k in range(i + 1, 6):
                v = v - L[k][i] * x[k]
            x[i] = v
    delta = np.array([-v for v in x], dtype=np.float64)
    if degenerate or not np.isfinite(delta).all():
        return None
    return delta


def update(pose, delta, pivot=None):
    """The Cayley retraction of delta = (v, omega) applied on the left of a column-major pose [16], about the pivot."""
    f = np.float64
    m = np.array(pose, dtype=np.float64).reshape(16)
    about = np.zeros(3) if pivot is None else np.asarray(pivot, dtype=np.float64).reshape(3)
    ax, ay, az = f(delta[3]) * f(0.5), f(delta[4]) * f(0.5), f(delta[5]) * f(0.5)
    s = f(1.0) + ((ax * ax + ay * ay) + az * az)
    k = f(2.0) / s
    D = [[f(1.0) - k * (ay * ay + az * az), k * (ax * ay - az), k * (ax * az + ay)],
         [k * (ax * ay + az), f(1.0) - k * (ax * ax + az * az), k * (ay * az - ax)],
         [k * (ax * az - ay), k * (ay * az + ax), f(1.0) - k * (ax * ax + ay * ay)]]
    out = m.copy()
    with np.errstate(all="ignore"):
        for c in range(3):
            for r in range(3):
                out[4 * c + r] = (D[r][0] * m[4 * c] + D[r][1] * m[4 * c + 1]) + D[r][2] * m[4 * c + 2]
        u = [m[12] - about[0], m[13] - about[1], m[14] - about[2]]
        for r in range(3):
            out[12 + r] = (((D[r][0] * u[0] + D[r][1] * u[1]) + D[r][2] * u[2]) + about[r]) + f(delta[r])
    return out


def align(sdf, resolution, points, poses, max_iterations=10, min_points=6, damping=0.0, max_residual=np.inf,
          target_distance=0.0, translation_tolerance=0.0, rotation_tolerance=0.0, pivot=None, grid_from_world=None,
          rotation=None):
    """-> CloudAlignment, one entry per pose of poses [B, 16]"""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 16)
    b = len(poses)
    out = CloudAlignment(np.empty((b, 16)), np.empty(b, np.uint8), np.empty(b, np.int32), np.empty(b, np.int32),
                         np.empty(b, np.int32), np.empty(b), np.empty(b, np.int32), np.empty((b, 27)), np.zeros((b, 6)))
    for i in range(b):
        pose = poses[i].copy()
        steps, last = 0, False
        evaluations = 0
        while True:
            ev = evaluate(sdf, resolution, points, pose, target_distance, max_residual, pivot, grid_from_world, rotation)
            evaluations += 1
            if ev.num_used < min_points:
                status = TOO_FEW
                break
            if last:
                status = CONVERGED
                break
            if steps >= max_iterations:
                status = ITERATION_LIMIT
                break
            delta = solve(ev.sums, damping)
            if delta is None:
                status = DEGENERATE
                break
            pose = update(pose, delta, pivot)
            out.last_step[i] = delta
            steps += 1
            last = (np.max(np.abs(delta[:3])) <= translation_tolerance and
                    np.max(np.abs(delta[3:])) <= rotation_tolerance)
        out.poses[i] = pose
        out.status[i] = status
        out.num_used[i], out.num_outside[i], out.num_rejected[i] = ev.num_used, ev.num_outside, ev.num_rejected
        out.sum_squared[i] = ev.sums[27]
        out.evaluations[i] = evaluations
        out.normal_equations[i] = ev.sums[:27]
    return out
