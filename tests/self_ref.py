"""CPU restatement of vgt_hip_check_self_collision and vgt_hip_self_collision_pairs (include/vgt_hip.h):
tests/kinematics_ref.py for the poses and for the summed form of the joint gradient, tests/body_ref.py's centre
expression (world_centres) for the centres.  Restated here are only the pair arithmetic -- every operator a numpy
temporary of its own --, the reductions, the status and the pair generator."""
import collections

import numpy as np

import body_ref
import kinematics_ref

CLEAR, COLLISION, NO_VALUE = 0, 1, 2

SelfCollisionChecks = collections.namedtuple(
    "SelfCollisionChecks", "status num_below num_without_value min_clearance min_pair min_direction joint_gradient "
    "fk_status pair_clearance")


def pair_clearances(spheres_xyzr, sphere_link, pairs, link_poses):
    """-> (clearance [B, P] (NaN without a value), e [B, P, 3], dist [B, P]); pairs with an index outside [0, S) are
    without a value."""
    xyzr = np.asarray(spheres_xyzr, dtype=np.float64).reshape(-1, 4)
    ab = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    poses = np.asarray(link_poses, dtype=np.float64)
    num, count = poses.shape[0], len(xyzr)
    centres, _ = body_ref.world_centres(xyzr, sphere_link, poses)               # [B, S, 3], NaN rows for bad links
    clearance = np.full((num, len(ab)), np.nan)
    e = np.full((num, len(ab), 3), np.nan)
    dist = np.full((num, len(ab)), np.nan)
    ok = np.zeros(len(ab), dtype=bool)
    if count > 0 and len(ab) > 0:
        ok = ((ab >= 0) & (ab < count)).all(axis=1)
    if ok.any() and num > 0:
        a, b = ab[ok, 0], ab[ok, 1]
        with np.errstate(all="ignore"):
            diff = centres[:, a, :] - centres[:, b, :]
            s0 = diff[..., 0] * diff[..., 0]
            s1 = diff[..., 1] * diff[..., 1]
            s2 = diff[..., 2] * diff[..., 2]
            d2 = s0 + s1
            d2 = d2 + s2
            root = np.sqrt(d2)
            c = root - xyzr[a, 3]
            c = c - xyzr[b, 3]
        e[:, ok], dist[:, ok], clearance[:, ok] = diff, root, c
    return clearance, e, dist


def reduce_pairs(tree, spheres_xyzr, sphere_link, pairs, link_poses, fk_status, clearance, e, dist,
                 minimum_clearance=0.0, no_value_is_collision=False):
    """The header's outputs from the per-pair values; tree None: no joint gradient."""
    xyzr = np.asarray(spheres_xyzr, dtype=np.float64).reshape(-1, 4)
    link = np.asarray(sphere_link, dtype=np.int32).reshape(-1)
    ab = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    num, count = clearance.shape[0], len(xyzr)
    if count == 0:                                                               # (the list is not looked at)
        clearance, e, dist = clearance[:, :0], e[:, :0], dist[:, :0]
    value = ~np.isnan(clearance)
    with np.errstate(invalid="ignore"):
        below = value & (clearance <= np.float64(minimum_clearance))
    num_below = below.sum(axis=1).astype(np.int32)
    num_without_value = (~value).sum(axis=1).astype(np.int32)
    min_clearance = np.full(num, np.nan)
    min_pair = np.full(num, -1, dtype=np.int32)
    min_direction = np.full((num, 3), np.nan)
    weight = np.zeros((num, count))
    gradient = np.zeros((num, count, 3))
    for i in range(num):
        if not value[i].any():
            continue
        least = np.min(clearance[i][value[i]])
        first = int(np.flatnonzero(value[i] & (clearance[i] == least))[0])      # (-0.0 == 0.0: the first of them)
        min_clearance[i] = clearance[i, first]
        min_pair[i] = first
        with np.errstate(all="ignore"):
            min_direction[i] = e[i, first] / dist[i, first]
        a, b = ab[first]
        weight[i, a] = weight[i, b] = 1.0
        gradient[i, a] = min_direction[i]
        gradient[i, b] = -min_direction[i]
    joint_gradient = None
    if tree is not None:
        if tree.num_joints > 0 and count > 0:
            joint_gradient = kinematics_ref.clearance_joint_gradient(tree, link_poses, xyzr, link, sphere_weight=weight,
                                                                     sphere_gradient=gradient)
        else:
            joint_gradient = np.zeros((num, tree.num_joints))
        joint_gradient[min_pair == -1] = np.nan
    collision = (num_below > 0) | (bool(no_value_is_collision) & (num_without_value > 0))
    status = np.where(collision, COLLISION, np.where(min_pair != -1, CLEAR, NO_VALUE)).astype(np.uint8)
    return SelfCollisionChecks(status, num_below, num_without_value, min_clearance, min_pair, min_direction,
                               joint_gradient, None if fk_status is None else np.asarray(fk_status, dtype=np.uint8),
                               clearance if count > 0 else None)


def check_self_collision_poses(spheres_xyzr, sphere_link, pairs, link_poses, tree=None, minimum_clearance=0.0,
                               no_value_is_collision=False, fk_status=None):
    poses = np.asarray(link_poses, dtype=np.float64)
    clearance, e, dist = pair_clearances(spheres_xyzr, sphere_link, pairs, poses)
    return reduce_pairs(tree, spheres_xyzr, sphere_link, pairs, poses, fk_status, clearance, e, dist, minimum_clearance,
                        no_value_is_collision)


def check_self_collision(spheres_xyzr, sphere_link, pairs, tree, joint_values, minimum_clearance=0.0,
                         no_value_is_collision=False, world_from_base=None, joint_limits=None):
    poses, fk_status = kinematics_ref.forward_kinematics(tree, joint_values, world_from_base, joint_limits)
    return check_self_collision_poses(spheres_xyzr, sphere_link, pairs, poses, tree, minimum_clearance,
                                      no_value_is_collision, fk_status)


def self_collision_pairs(sphere_link, num_links, parent=None, ignored_link_pairs=None, skip_adjacent=False):
    """-> pairs [P, 2] int32 in lexicographic order."""
    link = [int(k) for k in np.asarray(sphere_link).reshape(-1)]
    ignored = set()
    if ignored_link_pairs is not None:
        ignored = {frozenset((int(i), int(j))) for i, j in np.asarray(ignored_link_pairs).reshape(-1, 2)}
    up = None if parent is None else [int(k) for k in np.asarray(parent).reshape(-1)]
    out = []
    for a in range(len(link)):
        for b in range(a + 1, len(link)):
            la, lb = link[a], link[b]
            if la == lb or frozenset((la, lb)) in ignored:
                continue
            if skip_adjacent and up is not None and (up[la] == lb or up[lb] == la):
                continue
            out.append((a, b))
    return np.asarray(out, dtype=np.int32).reshape(-1, 2)
