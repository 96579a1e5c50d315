"""numpy restatement of vgt_hip_forward_kinematics and vgt_hip_clearance_joint_gradient (include/vgt_hip.h), operation by
operation: every operator below is one IEEE double operation, in the order the header gives, vectorised over the
configurations only.  The GPU tests hold every output bit-equal to this file; tests/test_kinematics_ref.py checks the
file itself (sin / cos accuracy, an independent route, central differences)."""
from fractions import Fraction
from math import factorial

import numpy as np

FIXED, REVOLUTE, PRISMATIC = 0, 1, 2
NOT_COMPUTABLE, OUTSIDE_LIMITS = 1, 2

TWO_OVER_PI = float.fromhex("0x1.45f306dc9c883p-1")
P1 = float.fromhex("0x1.921fb54400000p+0")
P2 = float.fromhex("0x1.0b4611a600000p-34")
P3 = float.fromhex("0x1.3198a2e037073p-69")
# the Taylor coefficients, correctly rounded (float(Fraction) rounds correctly)
S = {n: float(Fraction((-1) ** ((n - 1) // 2), factorial(n))) for n in range(3, 18, 2)}
C = {n: float(Fraction((-1) ** (n // 2), factorial(n))) for n in range(2, 17, 2)}
MAX_REVOLUTE = 2.0 ** 20


def sincos(q):
    """(sin, cos) of finite q with |q| <= 2^20, as the header defines them."""
    q = np.asarray(q, dtype=np.float64)
    k = np.rint(q * TWO_OVER_PI)
    r = ((q - k * P1) - k * P2) - k * P3
    z = r * r
    ps = np.full_like(z, S[17])
    for n in range(15, 2, -2):
        ps = ps * z + S[n]
    sin_r = r + (r * z) * ps
    pc = np.full_like(z, C[16])
    for n in range(14, 1, -2):
        pc = pc * z + C[n]
    cos_r = 1.0 + z * pc
    quadrant = k.astype(np.int64) & 3
    s = np.choose(quadrant, [sin_r, cos_r, -sin_r, -cos_r])
    c = np.choose(quadrant, [cos_r, -sin_r, -cos_r, sin_r])
    return s, c


class Tree:
    """The arrays of vgt_hip_kinematics_create, as numpy arrays."""

    def __init__(self, parent, joint_type, joint_index, axis, origin, num_joints):
        self.parent = np.ascontiguousarray(parent, dtype=np.int32).reshape(-1)
        self.joint_type = np.ascontiguousarray(joint_type, dtype=np.int32).reshape(-1)
        self.joint_index = np.ascontiguousarray(joint_index, dtype=np.int32).reshape(-1)
        self.axis = np.ascontiguousarray(axis, dtype=np.float64).reshape(-1, 3)
        self.origin = np.ascontiguousarray(origin, dtype=np.float64).reshape(-1, 16)
        self.num_links = len(self.parent)
        self.num_joints = int(num_joints)

    def arrays(self):
        return self.parent, self.joint_type, self.joint_index, self.axis, self.origin


def _rot(m, r, c):
    return m[..., 4 * c + r]


def _product(a, b):
    """A . B of two transforms given as [..., 16] column-major; only the twelve used elements are formed."""
    out = np.zeros(np.broadcast(a, b).shape, dtype=np.float64)
    for r in range(3):
        for c in range(3):
            out[..., 4 * c + r] = (_rot(a, r, 0) * _rot(b, 0, c) + _rot(a, r, 1) * _rot(b, 1, c)) + \
                _rot(a, r, 2) * _rot(b, 2, c)
        out[..., 12 + r] = ((_rot(a, r, 0) * b[..., 12] + _rot(a, r, 1) * b[..., 13]) + _rot(a, r, 2) * b[..., 14]) + \
            a[..., 12 + r]
    return out


def forward_kinematics(tree, joint_values, world_from_base=None, joint_limits=None):
    """-> (link_poses [B, L, 16] float64, status [B] uint8)."""
    q = np.ascontiguousarray(joint_values, dtype=np.float64)
    num = q.shape[0]
    q = q.reshape(num, tree.num_joints)
    poses = np.zeros((num, tree.num_links, 16), dtype=np.float64)
    status = np.zeros(num, dtype=np.uint8)
    base = None if world_from_base is None else np.asarray(world_from_base, dtype=np.float64).reshape(16)
    if joint_limits is not None and tree.num_joints:
        limits = np.asarray(joint_limits, dtype=np.float64).reshape(tree.num_joints, 2)
        outside = ((q < limits[None, :, 0]) | (q > limits[None, :, 1])).any(axis=1)
        status[outside] |= OUTSIDE_LIMITS
    with np.errstate(all="ignore"):
        for i in range(tree.num_links):
            origin = tree.origin[i]
            parent = int(tree.parent[i])
            if parent >= 0:
                f = _product(poses[:, parent], origin[None, :])
            elif base is not None:
                f = _product(np.broadcast_to(base, (num, 16)), origin[None, :])
            else:
                f = np.broadcast_to(origin, (num, 16)).copy()
            kind = int(tree.joint_type[i])
            x, y, z = tree.axis[i]
            t = f.copy()
            if kind != FIXED:
                v = q[:, tree.joint_index[i]]
                bad = ~np.isfinite(v)
                if kind == REVOLUTE:
                    bad |= np.abs(v) > MAX_REVOLUTE
                safe = np.where(bad, 0.0, v)
                if kind == REVOLUTE:
                    s, c = sincos(safe)
                    w = 1.0 - c
                    rot = np.zeros((num, 16), dtype=np.float64)
                    rot[:, 0] = c + (x * x) * w
                    rot[:, 4] = (x * y) * w - z * s
                    rot[:, 8] = (x * z) * w + y * s
                    rot[:, 1] = (x * y) * w + z * s
                    rot[:, 5] = c + (y * y) * w
                    rot[:, 9] = (y * z) * w - x * s
                    rot[:, 2] = (x * z) * w - y * s
                    rot[:, 6] = (y * z) * w + x * s
                    rot[:, 10] = c + (z * z) * w
                    t = _product(f, rot)
                    t[:, 12:15] = f[:, 12:15]
                else:
                    step = np.zeros((num, 16), dtype=np.float64)
                    step[:, 12] = x * safe
                    step[:, 13] = y * safe
                    step[:, 14] = z * safe
                    moved = _product(f, step)
                    t[:, 12:15] = moved[:, 12:15]
                t[bad] = np.nan
                status[bad] |= NOT_COMPUTABLE
            t[:, 3] = t[:, 7] = t[:, 11] = 0.0
            t[:, 15] = 1.0
            poses[:, i] = t
    return poses, status


def _sphere_centre(pose, xyzr):
    x, y, z = xyzr[0], xyzr[1], xyzr[2]
    return [((pose[r] * x + pose[4 + r] * y) + pose[8 + r] * z) + pose[12 + r] for r in range(3)]


def _walk(tree, poses_b, k, p, g, acc, weight):
    """Adds sphere terms along k, parent[k], ... into acc [J]; weight None: the worst-sphere form's plain sum."""
    i = k
    while i >= 0:
        kind = int(tree.joint_type[i])
        if kind != FIXED:
            m = poses_b[i]
            x, y, z = tree.axis[i]
            a = [(m[r] * x + m[4 + r] * y) + m[8 + r] * z for r in range(3)]
            if kind == REVOLUTE:
                d = [p[r] - m[12 + r] for r in range(3)]
                u = [a[1] * d[2] - a[2] * d[1], a[2] * d[0] - a[0] * d[2], a[0] * d[1] - a[1] * d[0]]
                term = (g[0] * u[0] + g[1] * u[1]) + g[2] * u[2]
            else:
                term = (g[0] * a[0] + g[1] * a[1]) + g[2] * a[2]
            j = int(tree.joint_index[i])
            acc[j] = acc[j] + (term if weight is None else weight * term)
        i = int(tree.parent[i])


def clearance_joint_gradient(tree, link_poses, sphere_xyzr, sphere_link, min_sphere=None, min_gradient=None,
                             sphere_weight=None, sphere_gradient=None):
    """-> joint_gradient [B, J] float64; exactly one of the pairs (min_sphere, min_gradient) and (sphere_weight,
    sphere_gradient) is given."""
    poses = np.asarray(link_poses, dtype=np.float64).reshape(-1, tree.num_links, 16)
    xyzr = np.asarray(sphere_xyzr, dtype=np.float64).reshape(-1, 4)
    link = np.asarray(sphere_link, dtype=np.int32).reshape(-1)
    num, count = poses.shape[0], len(link)
    out = np.zeros((num, tree.num_joints), dtype=np.float64)
    worst = min_sphere is not None
    assert worst != (sphere_weight is not None)
    with np.errstate(all="ignore"):
        for b in range(num):
            acc = [np.float64(0.0)] * tree.num_joints
            if worst:
                s = int(min_sphere[b])
                k = int(link[s]) if 0 <= s < count else -1
                if not 0 <= k < tree.num_links:
                    out[b] = np.nan
                    continue
                g = [np.float64(v) for v in np.asarray(min_gradient, dtype=np.float64).reshape(-1, 3)[b]]
                _walk(tree, poses[b], k, _sphere_centre(poses[b, k], xyzr[s]), g, acc, None)
            else:
                weights = np.asarray(sphere_weight, dtype=np.float64).reshape(num, count)
                gradients = np.asarray(sphere_gradient, dtype=np.float64).reshape(num, count, 3)
                for s in range(count):
                    w, k = weights[b, s], int(link[s])
                    if w == 0.0 or not 0 <= k < tree.num_links:
                        continue
                    g = [np.float64(v) for v in gradients[b, s]]
                    _walk(tree, poses[b], k, _sphere_centre(poses[b, k], xyzr[s]), g, acc, w)
            out[b] = acc
    return out
