"""CPU restatement of vgt_hip_check_motions (include/vgt_hip.h): the samples of every motion interpolated in numpy, every
operator a temporary of its own; tests/kinematics_ref.py and tests/body_ref.py on the flat samples; then the reduction per
motion by the header's rules.  Nothing of the kinematics or of the check is restated here."""
import collections

import numpy as np

import body_ref
import kinematics_ref

CLEAR, COLLISION, NO_VALUE, INVALID = 0, 1, 2, 3

MotionChecks = collections.namedtuple(
    "MotionChecks", "status first_collision min_clearance min_sample min_sphere min_gradient fk_status")

# what the per-sample calls return for the flat samples, in motion order: the reduction's input
Samples = collections.namedtuple("Samples", "status min_clearance min_sphere min_gradient fk_status")


def step_counts(num_steps, num_motions):
    if np.ndim(num_steps) == 0:
        return np.full(num_motions, int(num_steps), dtype=np.int64)
    return np.asarray(num_steps, dtype=np.int64).reshape(num_motions)


def interpolate(joint_from, joint_to, num_steps):
    """-> (q [sum(n + 1), J], first [E + 1]: motion e's samples are the rows first[e] ... first[e + 1] - 1)"""
    a = np.asarray(joint_from, dtype=np.float64)
    b = np.asarray(joint_to, dtype=np.float64)
    steps = step_counts(num_steps, len(a))
    first = np.concatenate([[0], np.cumsum(steps + 1)])
    q = np.empty((int(first[-1]), a.shape[1]))
    with np.errstate(invalid="ignore", over="ignore"):
        for e, n in enumerate(steps):
            rows = q[first[e]:first[e + 1]]
            rows[0] = a[e]
            for k in range(1, n):
                t = np.float64(k) / np.float64(n)
                d = b[e] - a[e]
                d = t * d
                rows[k] = a[e] + d
            if n > 0:
                rows[n] = b[e]
    return q, first


def reduce_motions(samples, first, stop_at_collision=False):
    """The header's reduction over the samples of each motion."""
    motions = len(first) - 1
    out = MotionChecks(np.empty(motions, np.uint8), np.empty(motions, np.int32), np.empty(motions, np.float64),
                       np.empty(motions, np.int32), np.empty(motions, np.int32), np.empty((motions, 3), np.float64),
                       np.empty(motions, np.uint8))
    for e in range(motions):
        lo, hi = int(first[e]), int(first[e + 1])
        status = samples.status[lo:hi]
        hits = np.flatnonzero(status == body_ref.COLLISION)
        first_collision = int(hits[0]) if len(hits) else -1
        if stop_at_collision and first_collision >= 0:
            hi = lo + first_collision + 1
            status = samples.status[lo:hi]
        clearance = samples.min_clearance[lo:hi]
        out.first_collision[e] = first_collision
        out.status[e] = (COLLISION if first_collision >= 0 else
                         NO_VALUE if (status == body_ref.NO_VALUE).any() else CLEAR)
        out.fk_status[e] = np.bitwise_or.reduce(samples.fk_status[lo:hi])
        candidate = ~np.isnan(clearance)
        if candidate.any():
            least = np.min(clearance[candidate])
            k = int(np.flatnonzero(candidate & (clearance == least))[0])            # (-0.0 == 0.0: the lowest k)
            out.min_clearance[e] = clearance[k]
            out.min_sample[e] = k
            out.min_sphere[e] = samples.min_sphere[lo + k]
            out.min_gradient[e] = samples.min_gradient[lo + k]
        else:
            out.min_clearance[e] = np.nan
            out.min_sample[e] = out.min_sphere[e] = -1
            out.min_gradient[e] = np.nan
    return out


def check_samples(oracle, sdf, resolution, spheres_xyzr, sphere_link, tree, joint_values, minimum_clearance=0.0,
                  outside_is_collision=False, grid_from_world=None, rotation=None, world_from_base=None,
                  joint_limits=None):
    """What vgt_hip_check_spheres_from_joints returns for joint_values, by the two existing restatements."""
    poses, fk_status = kinematics_ref.forward_kinematics(tree, joint_values, world_from_base, joint_limits)
    checks = body_ref.check_spheres(oracle, sdf, resolution, spheres_xyzr, sphere_link, poses, minimum_clearance,
                                    outside_is_collision, grid_from_world, rotation)
    return Samples(checks.status, checks.min_clearance, checks.min_sphere, checks.min_gradient, fk_status)


def check_motions(oracle, sdf, resolution, spheres_xyzr, sphere_link, tree, joint_from, joint_to, num_steps,
                  minimum_clearance=0.0, outside_is_collision=False, stop_at_collision=False, grid_from_world=None,
                  rotation=None, world_from_base=None, joint_limits=None):
    q, first = interpolate(joint_from, joint_to, num_steps)
    samples = check_samples(oracle, sdf, resolution, spheres_xyzr, sphere_link, tree, q, minimum_clearance,
                            outside_is_collision, grid_from_world, rotation, world_from_base, joint_limits)
    return reduce_motions(samples, first, stop_at_collision)
