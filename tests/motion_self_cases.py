"""Seeded inputs shared by tests/test_motion_self_ref.py and tests/test_gpu_motion_self.py: the motions of
tests/motion_cases.py -- the same 67 per case, with STEPS on both sides of every tile, the NaN row, the infinity row, the
2^20 row and the motion that goes nowhere -- with a pair list, and the answers of tests/motion_self_ref.py computed once
per case and kept read-only.  The environment's per-sample answers are those tests/motion_cases.py already holds.

Pairs: tests/self_ref.self_collision_pairs with parents skipped (a tree of one link: every pair of its spheres); of a
longer list MOST_PAIRS entries at even strides, so that no case has more than 2615 samples x 144 pairs.
self_minimum_clearance is the bits of a per-sample self min_clearance that occurs (the `<=` edge): the stated quantile of
the sorted finite per-sample self minima.  The cases of NO_VALUE_IS_COLLISION set
VGT_HIP_MOTION_SELF_NO_VALUE_IS_COLLISION.

The cases:
  BORROWED   cases of tests/motion_cases.py by name, with their field, model, limits, frame and threshold
  chain      the least chain of tests/kinematics_cases.py whose tile, with 6 spheres, is one sample
  no-spheres arm with S == 0 and a field; one pair is listed and never looked at: the self part is NO_VALUE everywhere
  field-less tests/self_cases.model(arm, 21), whose twins and triplets tie exactly and which has a NaN sphere, with
             tests/self_cases.pair_list; its radius-10 spheres make it unusable against the field, so there is none
  planted    arm-21 with both thresholds huge: sample 0 collides with cause 3

coverage() states what the cases must hit, so that none passes by hitting nothing; tests/test_motion_self_ref.py asserts
it."""
import collections
import functools

import numpy as np

import body_cases
import kinematics_cases
import motion_cases
import motion_ref
import motion_self_ref
import self_cases
import self_ref

RESOLUTION = motion_cases.RESOLUTION
TILE_BYTES, LDS_LIMIT, RECORD_BYTES = 16 * 1024, 64 * 1024, 1792
HUGE = 1.0e9
MOST_PAIRS = 144
NO_VALUE_IS_COLLISION = ("arm-70", "arm-21-planted")

# (name in tests/motion_cases.py, quantile of the self minima)
BORROWED = [("arm-21", 0.02), ("body-9", 0.02), ("body-9-odd", 0.02), ("arm-21-frame", 0.02), ("arm-70", 0.02),
            ("arm-257", 0.02), ("fixed1-2", 0.5)]


def tile_formula(num_links, num_spheres):
    """What include/vgt_hip.h says vgt_hip_motion_self_tile_samples gives (tests/test_gpu_motion_self.py holds the
    library to it), so that the cases do not depend on a built library."""
    if num_links <= 0 or num_spheres < 0 or 96 * num_links + 32 * num_spheres + RECORD_BYTES > LDS_LIMIT:
        return 0
    tile = 64
    while tile > 1 and (96 * num_links + 24 * num_spheres) * tile > TILE_BYTES:
        tile //= 2
    return tile


def one_per_tile_chain():
    return "chain-%d" % min(n for n in range(1, 200) if tile_formula(n, 6) == 1)


def names():
    return [name for name, _ in BORROWED] + [one_per_tile_chain() + "-6", "arm-0", "arm-21-field-less",
                                              "arm-21-planted"]


Case = collections.namedtuple(
    "Case", "name tree sdf xyzr link pairs joint_from joint_to num_steps minimum_clearance self_minimum_clearance "
            "outside_is_collision self_no_value_is_collision world_from_base joint_limits grid_from_world rotation "
            "samples self_samples first want want_stopped")


def pair_list(tree, link):
    if tree.num_links == 1:
        return np.asarray([(a, b) for a in range(len(link)) for b in range(a + 1, len(link))],
                          dtype=np.int32).reshape(-1, 2)
    pairs = self_ref.self_collision_pairs(link, tree.num_links, parent=tree.parent, skip_adjacent=True)
    if len(pairs) > MOST_PAIRS:
        pairs = np.ascontiguousarray(pairs[::len(pairs) // MOST_PAIRS][:MOST_PAIRS])
    return pairs


def _self_samples(tree, xyzr, link, pairs, q, base, limits, quantile, flag):
    """-> (self_minimum_clearance, the per-sample answers at it); quantile None: HUGE."""
    poses, fk_status = self_ref.kinematics_ref.forward_kinematics(tree, q, base, limits)
    clearance, e, dist = self_ref.pair_clearances(xyzr, link, pairs, poses)

    def at(threshold):
        return self_ref.reduce_pairs(None, xyzr, link, pairs, poses, fk_status, clearance, e, dist, threshold, flag)

    if quantile is None:
        return HUGE, at(HUGE)
    finite = np.sort(at(0.0).min_clearance)
    finite = finite[np.isfinite(finite)]
    threshold = float(finite[int(quantile * (len(finite) - 1))]) if len(finite) else 0.0
    return threshold, at(threshold)


@functools.lru_cache(maxsize=None)
def case(index):
    from oracle import oracle as O
    name = names()[index]
    flag = name in NO_VALUE_IS_COLLISION or name.startswith("chain")
    grid_from_world = rotation = limits = None
    base = motion_cases.world_from_base()
    if index < len(BORROWED):
        m = motion_cases.case(motion_cases.names().index(name))
        tree, sdf, xyzr, link = m.tree, m.sdf, m.xyzr, m.link
        joint_from, joint_to, num_steps, first = m.joint_from, m.joint_to, m.num_steps, m.first
        minimum, outside, base, limits = m.minimum_clearance, m.outside_is_collision, m.world_from_base, m.joint_limits
        grid_from_world, rotation, samples = m.grid_from_world, m.rotation, m.samples
        pairs, quantile = pair_list(tree, link), BORROWED[index][1]
        q, again = motion_ref.interpolate(joint_from, joint_to, num_steps)
        assert np.array_equal(again, first)
    else:
        kind = name.rsplit("-", 1)[-1]
        tree = kinematics_cases.tree(one_per_tile_chain() if name.startswith("chain") else "arm")
        joint_from, joint_to = motion_cases.endpoints(tree.num_joints)
        num_steps = np.array([motion_cases.STEPS[e % len(motion_cases.STEPS)] for e in range(motion_cases.NUM_MOTIONS)],
                             dtype=np.int32)
        q, first = motion_ref.interpolate(joint_from, joint_to, num_steps)
        sdf, outside, quantile, minimum = body_cases.field(False), False, 0.02, None
        if kind == "less":
            xyzr, link, planted = self_cases.model(tree, 21)
            # (the triplets at -9.8, a constant; the twins at about -10 + |t - c|, which moves: they share the samples)
            xyzr[list(planted[3:6]), 3] = 4.9
            pairs, sdf, limits = self_cases.pair_list(tree, link, planted), None, kinematics_cases.limits(tree.num_joints)
            quantile = 0.02
        elif kind == "0":
            xyzr, link, pairs = np.zeros((0, 4)), np.zeros(0, np.int32), np.array([[0, 1]], np.int32)
        else:
            xyzr, link = kinematics_cases.sphere_model(tree, 6 if name.startswith("chain") else 21, 31)
            pairs = pair_list(tree, link)
            if kind == "planted":
                quantile, minimum = None, HUGE
        samples = None
        if sdf is not None:
            def samples_at(threshold):
                return motion_ref.check_samples(O, sdf, RESOLUTION, xyzr, link, tree, q, threshold, outside, None, None,
                                                base, limits)
            if minimum is None:
                finite = np.sort(samples_at(0.0).min_clearance)
                finite = finite[np.isfinite(finite)]
                minimum = float(finite[int(0.01 * (len(finite) - 1))]) if len(finite) else 0.0
            samples = samples_at(minimum)
        else:
            minimum = 0.0
    self_minimum, self_samples = _self_samples(tree, xyzr, link, pairs, q, base, limits, quantile, flag)
    want = motion_self_ref.reduce_with_self(samples, self_samples, first, False)
    want_stopped = motion_self_ref.reduce_with_self(samples, self_samples, first, True)
    arrays = [xyzr, link, pairs, joint_from, joint_to, base, first] + list(want) + list(want_stopped)
    arrays += [a for a in self_samples if isinstance(a, np.ndarray)]
    arrays += [a for a in (num_steps, limits) if isinstance(a, np.ndarray)]
    for a in arrays:
        a.setflags(write=False)
    return Case(name, tree, sdf, xyzr, link, pairs, joint_from, joint_to, num_steps, minimum, self_minimum, outside, flag,
                base, limits, grid_from_world, rotation, samples, self_samples, first, want, want_stopped)


def environment_alone(c, stop):
    """What vgt_hip_check_motions gives for the case: tests/motion_ref.py's reduction of the same samples."""
    return motion_ref.reduce_motions(c.samples, c.first, stop)


Coverage = collections.namedtuple(
    "Coverage", "environment_only self_only both first_collision_moved stop_moves_self_minimum self_no_value_alone "
                "self_threshold_occurs")


def coverage(index):
    """Counts over the case's motions: the cause of the first collision (1, 2, 3); first_collision other than
    vgt_hip_check_motions'; self_min_sample other with the stop flag than without; NO_VALUE where no sample's
    environment part (if there is one) is NO_VALUE; and the samples whose self min_clearance is self_minimum_clearance."""
    c = case(index)
    want, stopped = c.want, c.want_stopped
    cause = want.collision_cause
    moved = alone = 0
    if c.samples is not None:
        moved = int((environment_alone(c, False).first_collision != want.first_collision).sum())
    for e in np.flatnonzero(want.status == motion_self_ref.NO_VALUE):
        lo, hi = int(c.first[e]), int(c.first[e + 1])
        from_self = (c.self_samples.status[lo:hi] == self_ref.NO_VALUE).any()
        from_field = c.samples is not None and (c.samples.status[lo:hi] == motion_ref.body_ref.NO_VALUE).any()
        alone += bool(from_self and not from_field)
    return Coverage(int((cause == 1).sum()), int((cause == 2).sum()), int((cause == 3).sum()), moved,
                    int((want.self_min_sample != stopped.self_min_sample).sum()), alone,
                    int((c.self_samples.min_clearance == c.self_minimum_clearance).sum()))
