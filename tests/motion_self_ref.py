"""CPU restatement of vgt_hip_check_motions_with_self (include/vgt_hip.h): tests/motion_ref.py's interpolation and
per-sample environment check and tests/self_ref.py's self-collision check on the flat samples, then the reduction per
motion by the header's rules.  Only that reduction is restated here."""
import collections

import numpy as np

import body_ref
import motion_ref
import self_ref

CLEAR, COLLISION, NO_VALUE, INVALID = 0, 1, 2, 3
CAUSE_ENVIRONMENT, CAUSE_SELF = 1, 2

MotionSelfChecks = collections.namedtuple(
    "MotionSelfChecks", "status first_collision collision_cause min_clearance min_sample min_sphere min_gradient "
    "self_min_clearance self_min_sample self_min_pair fk_status")

# the fields vgt_hip_check_motions has too
SHARED = motion_ref.MotionChecks._fields
ENVIRONMENT = ("min_clearance", "min_sample", "min_sphere", "min_gradient")


def _least(values):
    """-> (k, values[k]) of the least non-NaN value, ties under == to the lowest k; (-1, NaN) without one."""
    candidate = ~np.isnan(values)
    if not candidate.any():
        return -1, np.nan
    least = np.min(values[candidate])
    k = int(np.flatnonzero(candidate & (values == least))[0])                        # (-0.0 == 0.0: the lowest k)
    return k, values[k]


def reduce_with_self(samples, self_samples, first, stop=False):
    """The header's reduction.  samples: motion_ref.Samples of the flat samples, or None without an environment part;
    self_samples: what self_ref.check_self_collision returns for them, or None without a self part."""
    assert samples is not None or self_samples is not None
    motions = len(first) - 1
    out = MotionSelfChecks(np.empty(motions, np.uint8), np.empty(motions, np.int32), np.empty(motions, np.uint8),
                           np.empty(motions, np.float64), np.empty(motions, np.int32), np.empty(motions, np.int32),
                           np.empty((motions, 3), np.float64), np.empty(motions, np.float64),
                           np.empty(motions, np.int32), np.empty(motions, np.int32), np.empty(motions, np.uint8))
    total = int(first[-1])
    cause = np.zeros(total, np.uint8)
    no_value = np.zeros(total, bool)
    if samples is not None:
        cause |= np.where(samples.status == body_ref.COLLISION, CAUSE_ENVIRONMENT, 0).astype(np.uint8)
        no_value |= samples.status == body_ref.NO_VALUE
    if self_samples is not None:
        cause |= np.where(self_samples.status == self_ref.COLLISION, CAUSE_SELF, 0).astype(np.uint8)
        no_value |= self_samples.status == self_ref.NO_VALUE
    no_value &= cause == 0
    fk_status = samples.fk_status if samples is not None else self_samples.fk_status
    if samples is not None and self_samples is not None:
        assert np.array_equal(samples.fk_status, self_samples.fk_status)
    for e in range(motions):
        lo, hi = int(first[e]), int(first[e + 1])
        hits = np.flatnonzero(cause[lo:hi] != 0)
        first_collision = int(hits[0]) if len(hits) else -1
        if stop and first_collision >= 0:
            hi = lo + first_collision + 1
        out.first_collision[e] = first_collision
        out.collision_cause[e] = cause[lo + first_collision] if first_collision >= 0 else 0
        out.status[e] = COLLISION if first_collision >= 0 else NO_VALUE if no_value[lo:hi].any() else CLEAR
        out.fk_status[e] = np.bitwise_or.reduce(fk_status[lo:hi])
        k, value = _least(samples.min_clearance[lo:hi]) if samples is not None else (-1, np.nan)
        out.min_clearance[e], out.min_sample[e] = value, k
        out.min_sphere[e] = samples.min_sphere[lo + k] if k >= 0 else -1
        out.min_gradient[e] = samples.min_gradient[lo + k] if k >= 0 else np.nan
        k, value = _least(self_samples.min_clearance[lo:hi]) if self_samples is not None else (-1, np.nan)
        out.self_min_clearance[e], out.self_min_sample[e] = value, k
        out.self_min_pair[e] = self_samples.min_pair[lo + k] if k >= 0 else -1
    return out


def check_self_samples(spheres_xyzr, sphere_link, pairs, tree, joint_values, self_minimum_clearance=0.0,
                       self_no_value_is_collision=False, world_from_base=None, joint_limits=None):
    """What vgt_hip_check_self_collision returns for joint_values (without its gradient: tree=None in the reduction)."""
    poses, fk_status = self_ref.kinematics_ref.forward_kinematics(tree, joint_values, world_from_base, joint_limits)
    return self_ref.check_self_collision_poses(spheres_xyzr, sphere_link, pairs, poses, None, self_minimum_clearance,
                                               self_no_value_is_collision, fk_status)


def check_motions_with_self(oracle, sdf, resolution, spheres_xyzr, sphere_link, pairs, tree, joint_from, joint_to,
                            num_steps, minimum_clearance=0.0, self_minimum_clearance=0.0, outside_is_collision=False,
                            stop_at_collision=False, self_no_value_is_collision=False, grid_from_world=None,
                            rotation=None, world_from_base=None, joint_limits=None):
    """sdf None: no environment part; pairs None or empty: no self part."""
    q, first = motion_ref.interpolate(joint_from, joint_to, num_steps)
    samples = self_samples = None
    if sdf is not None:
        samples = motion_ref.check_samples(oracle, sdf, resolution, spheres_xyzr, sphere_link, tree, q, minimum_clearance,
                                           outside_is_collision, grid_from_world, rotation, world_from_base, joint_limits)
    if pairs is not None and len(pairs) > 0:
        self_samples = check_self_samples(spheres_xyzr, sphere_link, pairs, tree, q, self_minimum_clearance,
                                          self_no_value_is_collision, world_from_base, joint_limits)
    if samples is None and self_samples is None:
        raise ValueError("neither a field nor a pair")
    return reduce_with_self(samples, self_samples, first, stop_at_collision)
