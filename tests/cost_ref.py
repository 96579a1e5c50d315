"""CPU restatement of vgt_hip_clearance_cost (include/vgt_hip.h): tests/kinematics_ref.py for the poses, tests/body_ref.py
for every sphere's clearance and gradient, the hinge in numpy with every operator a temporary of its own and the
branches in the header's order, the NaN-gradient rule, tests/kinematics_ref.py's summed form for the joint gradient and a
Python loop for the ordered cost sum.  Nothing of the kinematics, of the check or of the gradient's term is restated."""
import collections

import numpy as np

import body_ref
import kinematics_ref

ClearanceCosts = collections.namedtuple(
    "ClearanceCosts", "cost joint_gradient num_active num_outside num_without_gradient fk_status")

# what the two restatements give per sphere, and what the hinge makes of it: kept by the cases for their own assertions
Spheres = collections.namedtuple("Spheres", "poses fk_status clearance gradient c w")


def hinge(d, margin):
    """-> (c, w) of the header's table for clearances d (any shape); c is NaN and w 0 where d is NaN."""
    d = np.asarray(d, dtype=np.float64)
    eps = np.float64(margin)
    c = np.full(d.shape, np.nan)
    w = np.zeros(d.shape)
    with np.errstate(all="ignore"):
        value = ~np.isnan(d)
        below = value & (d < 0.0)
        inside = value & ~below & (d <= eps)
        beyond = value & ~below & ~inside
        half = eps * np.float64(0.5)
        c[below] = half - d[below]
        w[below] = -1.0
        t = d[inside] - eps
        square = t * t
        square = square * np.float64(0.5)
        c[inside] = square / eps
        w[inside] = t / eps
        c[beyond] = 0.0
    return c, w


def spheres(oracle, sdf, resolution, spheres_xyzr, sphere_link, tree, joint_values, margin, grid_from_world=None,
            rotation=None, world_from_base=None, joint_limits=None):
    poses, fk_status = kinematics_ref.forward_kinematics(tree, joint_values, world_from_base, joint_limits)
    checks = body_ref.check_spheres(oracle, sdf, resolution, spheres_xyzr, sphere_link, poses, 0.0, False,
                                    grid_from_world, rotation)
    num = len(poses)
    clearance = np.asarray(checks.sphere_clearance, dtype=np.float64).reshape(num, -1)
    gradient = np.asarray(checks.sphere_gradient, dtype=np.float64).reshape(num, -1, 3)
    c, w = hinge(clearance, margin)
    return Spheres(poses, fk_status, clearance, gradient, c, w)


def reduce_spheres(tree, spheres_xyzr, sphere_link, per_sphere):
    """The header's outputs from the per-sphere values."""
    poses, fk_status, clearance, gradient, c, w = per_sphere
    num, count = clearance.shape
    value = ~np.isnan(clearance)
    active = value & (w != 0.0)
    without_gradient = active & np.isnan(gradient).any(axis=2)
    weight = np.where(without_gradient, 0.0, w)
    if tree.num_joints > 0:
        joint_gradient = kinematics_ref.clearance_joint_gradient(tree, poses, spheres_xyzr, sphere_link,
                                                                 sphere_weight=weight, sphere_gradient=gradient)
    else:
        joint_gradient = np.zeros((num, 0))
    cost = np.empty(num)
    with np.errstate(all="ignore"):
        for b in range(num):
            acc = np.float64(0.0)
            for s in range(count):
                if value[b, s]:
                    acc = acc + c[b, s]
            cost[b] = acc
    return ClearanceCosts(cost, joint_gradient, active.sum(axis=1).astype(np.int32),
                          (~value).sum(axis=1).astype(np.int32), without_gradient.sum(axis=1).astype(np.int32),
                          np.asarray(fk_status, dtype=np.uint8))


def clearance_cost(oracle, sdf, resolution, spheres_xyzr, sphere_link, tree, joint_values, margin, grid_from_world=None,
                   rotation=None, world_from_base=None, joint_limits=None):
    per_sphere = spheres(oracle, sdf, resolution, spheres_xyzr, sphere_link, tree, joint_values, margin, grid_from_world,
                         rotation, world_from_base, joint_limits)
    return reduce_spheres(tree, spheres_xyzr, sphere_link, per_sphere)
