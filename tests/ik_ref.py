"""numpy restatement of vgt_hip_solve_ik (include/vgt_hip.h), operation by operation: every operator below is one IEEE
double operation, in the order the header gives.  The poses are tests/kinematics_ref.py's.  Every problem is solved on
its own -- the arrays below only run the problems that are still live side by side, element by element, and no operation
mixes two of them.  The GPU tests hold every output bit-equal to this file; tests/test_ik_ref.py checks the file itself
(columns against central differences, convergence, the planted rows)."""
import collections

import numpy as np

import kinematics_ref as R

CONVERGED, ITERATION_LIMIT, DEGENERATE, NOT_COMPUTABLE = 0, 1, 2, 3

IkSolutions = collections.namedtuple("IkSolutions", "joints status iterations error tip_pose fk_status")


def chain_of(tree, tip_link):
    """The links on the way from the base to the tip, base first."""
    chain = []
    i = int(tip_link)
    while i >= 0:
        chain.append(i)
        i = int(tree.parent[i])
    return chain[::-1]


def moving_links(tree, tip_link):
    """The chain's links that are not FIXED, in walk order: from the tip to the base."""
    return [i for i in chain_of(tree, tip_link)[::-1] if int(tree.joint_type[i]) != R.FIXED]


def shared_column(tree, tip_link):
    """(link, link) of two moving chain links that read one column (the pair the call names when it refuses), or None."""
    seen = {}
    for i in chain_of(tree, tip_link):
        if int(tree.joint_type[i]) == R.FIXED:
            continue
        j = int(tree.joint_index[i])
        if j in seen:
            return seen[j], i
        seen[j] = i
    return None


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def evaluate(tree, tip_link, q, targets, world_from_base=None):
    """-> (poses [n, L, 16], e: six arrays [n], trace [n], not computable [n] bool) for the rows q [n, J]."""
    poses, _ = R.forward_kinematics(tree, q, world_from_base, None)
    bad = np.zeros(len(q), dtype=bool)
    for i in moving_links(tree, tip_link):
        v = q[:, tree.joint_index[i]]
        bad |= ~np.isfinite(v)
        if int(tree.joint_type[i]) == R.REVOLUTE:
            bad |= np.abs(v) > R.MAX_REVOLUTE
    m = poses[:, tip_link]
    e = [targets[:, 12 + r] - m[:, 12 + r] for r in range(3)]
    x = [_cross([m[:, 4 * c + r] for r in range(3)], [targets[:, 4 * c + r] for r in range(3)]) for c in range(3)]
    e += [((x[0][r] + x[1][r]) + x[2][r]) * 0.5 for r in range(3)]
    d = [_dot([m[:, 4 * c + r] for r in range(3)], [targets[:, 4 * c + r] for r in range(3)]) for c in range(3)]
    trace = (d[0] + d[1]) + d[2]
    return poses, e, trace, bad


def columns(tree, tip_link, poses, weights):
    """The weighted columns, one list of six arrays [n] per moving chain link, in walk order."""
    p = [poses[:, tip_link, 12 + r] for r in range(3)]
    out = []
    for i in moving_links(tree, tip_link):
        m = poses[:, i]
        x, y, z = tree.axis[i]
        a = [(m[:, r] * x + m[:, 4 + r] * y) + m[:, 8 + r] * z for r in range(3)]
        if int(tree.joint_type[i]) == R.REVOLUTE:
            d = [p[r] - m[:, 12 + r] for r in range(3)]
            c = _cross(a, d) + a
        else:
            c = a + [np.zeros(len(m))] * 3
        out.append([weights[k] * c[k] for k in range(6)])
    return out


def solve6(A, b):
    """The LDL^T sequence of vgt_hip_align_points' "solve" on A (A[j][k] for j <= k is read) and b, each entry an array
    [n] -> (x: six arrays, degenerate [n] bool)."""
    n = len(b[0])
    L = [[None] * 6 for _ in range(6)]
    D = [None] * 6
    degenerate = np.zeros(n, dtype=bool)
    for j in range(6):
        d = A[j][j]
        for k in range(j):
            d = d - (L[j][k] * L[j][k]) * D[k]
        D[j] = d
        degenerate |= ~(d > 0.0)
        for i in range(j + 1, 6):
            l = A[j][i]
            for k in range(j):
                l = l - (L[i][k] * L[j][k]) * D[k]
            L[i][j] = l / d
    y = [None] * 6
    for i in range(6):
        v = b[i]
        for k in range(i):
            v = v - L[i][k] * y[k]
        y[i] = v
    x = [None] * 6
    for i in range(5, -1, -1):
        v = y[i] / D[i]
        for k in range(i + 1, 6):
            v = v - L[k][i] * x[k]
        x[i] = v
    for i in range(6):
        degenerate |= ~np.isfinite(x[i])
    return x, degenerate


def solve_ik(tree, tip_link, targets, seeds, seeds_per_target=1, world_from_base=None, joint_limits=None,
             task_weights=None, max_iterations=50, damping=0.01, max_step=0.5, position_tolerance=1e-6,
             rotation_tolerance=1e-6):
    """-> IkSolutions(joints [B, J], status [B] uint8, iterations [B] int32, error [B, 6], tip_pose [B, 16],
    fk_status [B] uint8) for targets [T, 16] and seeds [T * seeds_per_target, J]."""
    assert shared_column(tree, tip_link) is None
    targets = np.ascontiguousarray(targets, dtype=np.float64).reshape(-1, 16)
    num = len(targets) * int(seeds_per_target)
    q = np.array(seeds, dtype=np.float64).reshape(num, tree.num_joints)
    aim = np.repeat(targets, int(seeds_per_target), axis=0)
    w = np.ones(6) if task_weights is None else np.asarray(task_weights, dtype=np.float64).reshape(6)
    limits = None if joint_limits is None else np.asarray(joint_limits, dtype=np.float64).reshape(tree.num_joints, 2)
    tolerance = [position_tolerance] * 3 + [rotation_tolerance] * 3
    damping, max_step = np.float64(damping), np.float64(max_step)
    moving = moving_links(tree, tip_link)

    status = np.zeros(num, dtype=np.uint8)
    iterations = np.zeros(num, dtype=np.int32)
    error = np.zeros((num, 6), dtype=np.float64)
    tip_pose = np.zeros((num, 16), dtype=np.float64)
    fk_status = np.zeros(num, dtype=np.uint8)
    live = np.arange(num)
    with np.errstate(all="ignore"):
        while len(live):
            rows = q[live]
            poses, e, trace, bad = evaluate(tree, tip_link, rows, aim[live], world_from_base)
            converged = np.ones(len(live), dtype=bool)
            for i in range(6):
                if w[i] != 0.0:
                    converged &= np.abs(e[i]) <= tolerance[i]
            if w[3] != 0.0 and w[4] != 0.0 and w[5] != 0.0:
                converged &= trace > 1.0
            A = [[None] * 6 for _ in range(6)]
            cols = columns(tree, tip_link, poses, w)
            for j in range(6):
                for k in range(j, 6):
                    acc = np.zeros(len(live))
                    for c in cols:
                        acc = acc + c[j] * c[k]
                    A[j][k] = acc
                A[j][j] = A[j][j] + damping * damping
            y, degenerate = solve6(A, [w[i] * e[i] for i in range(6)])
            stop = np.where(bad, NOT_COMPUTABLE,
                            np.where(converged, CONVERGED,
                                     np.where(iterations[live] >= max_iterations, ITERATION_LIMIT,
                                              np.where(degenerate, DEGENERATE, -1))))
            done = stop >= 0
            at = live[done]
            status[at] = stop[done]
            error[at] = np.stack(e, axis=1)[done]
            tip_pose[at] = poses[done, tip_link]
            fk_status[at] = np.where(bad[done], R.NOT_COMPUTABLE, 0)
            if limits is not None and tree.num_joints:
                outside = ((rows[done] < limits[None, :, 0]) | (rows[done] > limits[None, :, 1])).any(axis=1)
                fk_status[at] |= np.where(outside, R.OUTSIDE_LIMITS, 0).astype(np.uint8)
            # the step of the problems that go on
            go = ~done
            dq = [((((c[0] * y[0] + c[1] * y[1]) + c[2] * y[2]) + c[3] * y[3]) + c[4] * y[4]) + c[5] * y[5] for c in cols]
            mx = np.zeros(len(live))
            for v in dq:
                mx = np.where(np.abs(v) > mx, np.abs(v), mx)
            scale = max_step / mx
            for i, v in zip(moving, dq):
                v = np.where(mx > max_step, v * scale, v)
                j = int(tree.joint_index[i])
                new = rows[:, j] + v
                if limits is not None:
                    new = np.where(new < limits[j, 0], limits[j, 0], new)
                    new = np.where(new > limits[j, 1], limits[j, 1], new)
                rows[:, j] = new
            q[live[go]] = rows[go]
            iterations[live[go]] += 1
            live = live[go]
    return IkSolutions(q, status, iterations, error, tip_pose, fk_status)
