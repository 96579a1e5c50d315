"""Seeded inputs shared by tests/test_self_ref.py and tests/test_gpu_self.py: configurations of the trees of
tests/kinematics_cases.py carrying sphere models with a pair list, with the answers of tests/self_ref.py computed once per
case and kept read-only.

A planted case (S >= 21) ends its model with seven planted spheres, after S - 7 random ones:
  t            radius 0, on link 0
  c, c'        twins (one link -- the last one --, one centre, one radius 10): the pairs (t, c) and (t, c') tie exactly,
               at about -10 + |t - c|, which moves with the configuration where a joint lies in between
  u, u', u''   triplets on the middle link: the pairs (u, u'') and (u', u'') have coincident centres, tie exactly at
               -2 R and have a NaN direction.  R is chosen from the restatement's own distances so that the triplets are
               the minimum in about half of the configurations and the twins in the others (a tree without joints, or
               fewer than four configurations with a value: R = 10, the triplets always)
  n            a sphere with a NaN coordinate: its pairs are without a value in every configuration
The list is what the pair generator gives for the random spheres (those on different links) followed by the planted pairs
(t, c), (t, c'), (t, n), (u, u''), (u', u'') and (t, c) once more -- duplicates are allowed --, so that the ties are
between neighbours in the list, between its end and its middle, and between three entries.
minimum_clearance is the bits of a clearance that occurs among the random spheres (EDGE), or 0.
Joint values are cost_cases.joint_values: uniform in +-1 with planted rows -- a NaN, an infinity, a value beyond 2^20, a
row of zeros.  Every second case passes joint limits, every third sets no_value_is_collision.

coverage() states what the cases must hit, so that none passes by hitting nothing; tests/test_self_ref.py asserts it."""
import collections
import functools

import numpy as np

import cost_cases
import kinematics_cases
import motion_cases
import self_ref

NUM_CONFIGURATIONS = 67
SEED = 9
EDGE = "edge"
PLANTED = 7
TILE_BYTES, LDS_LIMIT = 16 * 1024, 64 * 1024


def tile_formula(num_links, num_spheres):
    """What include/vgt_hip.h says vgt_hip_self_collision_tile_samples gives (tests/test_gpu_self.py holds the library
    to it), so that the cases do not depend on a built library."""
    if num_links <= 0 or 96 * num_links + 32 * num_spheres + 256 > LDS_LIMIT:
        return 0
    tile = 64
    while tile > 1 and (96 * num_links + 24 * num_spheres) * tile > TILE_BYTES:
        tile //= 2
    return tile


def one_per_tile_chain():
    """The least chain of kinematics_cases whose tile, with 21 spheres, is one configuration."""
    return "chain-%d" % min(n for n in range(1, 200) if tile_formula(n, 21) == 1)


def deep_chain():
    return kinematics_cases.deep_names()[3]


def _cases():
    t = tile_formula(8, 21)
    # (tree, S, B, minimum_clearance)
    out = [
        ("fixed1", 21, NUM_CONFIGURATIONS, EDGE),
        ("arm", 1, NUM_CONFIGURATIONS, 0.0),
        ("arm", 2, NUM_CONFIGURATIONS, 0.0),
        ("arm", 21, NUM_CONFIGURATIONS, EDGE),
        ("arm", 65, NUM_CONFIGURATIONS, EDGE),
        ("arm", 257, NUM_CONFIGURATIONS, EDGE),
        ("body", 21, NUM_CONFIGURATIONS, EDGE),
        ("body", 65, NUM_CONFIGURATIONS, 0.0),
        (deep_chain(), 21, NUM_CONFIGURATIONS, EDGE),
        (one_per_tile_chain(), 21, 9, EDGE),
        ("arm", 0, NUM_CONFIGURATIONS, 0.0),
    ]
    out += [("arm", 21, b, EDGE) for b in (1, t - 1, t, t + 1, 257)]
    return out


CASES = _cases()

Case = collections.namedtuple(
    "Case", "name tree xyzr link pairs joint_values minimum_clearance no_value_is_collision world_from_base joint_limits "
    "poses fk_status planted want")


def names():
    out = []
    for tree, s, b, minimum in CASES:
        name = "%s-%d" % (tree, s)
        if b != NUM_CONFIGURATIONS:
            name += "-B%d" % b
        if minimum != EDGE:
            name += "-m%g" % minimum
        out.append(name)
    return out


def model(tree, num_spheres):
    """-> (xyzr, link, planted): planted is None or the indices (t, c, c', u, u', u'', n); the triplets' radius is 10."""
    if num_spheres == 0:
        return np.zeros((0, 4)), np.zeros(0, np.int32), None
    if num_spheres < PLANTED + 2:
        xyzr, link = kinematics_cases.sphere_model(tree, num_spheres, 41)
        return xyzr, link, None
    free = num_spheres - PLANTED
    xyzr, link = kinematics_cases.sphere_model(tree, num_spheres, 41)
    xyzr, link = xyzr.copy(), link.copy()
    last, middle = tree.num_links - 1, tree.num_links // 2
    t, c, c2, u, u2, u3, n = range(free, num_spheres)
    xyzr[t], link[t] = [0.05, -0.02, 0.03, 0.0], 0
    xyzr[c] = xyzr[c2] = [0.11, 0.07, -0.05, 10.0]
    link[c] = link[c2] = last
    xyzr[u] = xyzr[u2] = xyzr[u3] = [-0.03, 0.02, 0.06, 10.0]
    link[u] = link[u2] = link[u3] = middle
    xyzr[n], link[n] = [np.nan, 0.0, 0.0, 0.01], 0
    return xyzr, link, (t, c, c2, u, u2, u3, n)


def pair_list(tree, link, planted):
    if planted is None:
        return self_ref.self_collision_pairs(link, tree.num_links)
    pairs = self_ref.self_collision_pairs(link[:planted[0]], tree.num_links)
    if tree.num_links == 1:
        # (one link: the generator gives nothing; every pair of the random spheres instead)
        pairs = np.asarray([(a, b) for a in range(planted[0]) for b in range(a + 1, planted[0])], dtype=np.int32)
    t, c, c2, u, u2, u3, n = planted
    extra = [(t, c), (t, c2), (t, n), (u, u3), (u2, u3), (t, c)]
    return np.concatenate([pairs, np.asarray(extra, dtype=np.int32)]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def case(index):
    tree_name, num_spheres, num, minimum = CASES[index]
    tree = kinematics_cases.tree(tree_name)
    xyzr, link, planted = model(tree, num_spheres)
    pairs = pair_list(tree, link, planted)
    q = cost_cases.joint_values(num, tree.num_joints, SEED)
    limits = kinematics_cases.limits(tree.num_joints) if index % 2 == 1 else None
    base = motion_cases.world_from_base()
    flag = index % 3 == 2
    poses, fk_status = self_ref.kinematics_ref.forward_kinematics(tree, q, base, limits)
    if planted is not None:
        t, c, c2, u, u2, u3, n = planted
        # the least clearance of every other pair (about -10: t against a twin)
        xyzr[[u, u2, u3], 3] = 5.0
        others = [i for i, (a, b) in enumerate(pairs.tolist()) if not (a in (u, u2) and b == u3)]
        clearance, _, _ = self_ref.pair_clearances(xyzr, link, pairs[others], poses)
        with np.errstate(all="ignore"):
            least = np.unique(np.nanmin(clearance[~np.isnan(clearance).all(axis=1)], axis=1))
        if tree.num_joints > 0 and len(least) >= 4:
            # -2 R = the median of those: the triplets and the twins share the configurations
            xyzr[[u, u2, u3], 3] = -float(np.median(least)) * 0.5
        else:
            xyzr[[u, u2, u3], 3] = 10.0
    clearance, e, dist = self_ref.pair_clearances(xyzr, link, pairs, poses)
    if minimum == EDGE:
        among = clearance[:, :len(pairs) - 6] if planted is not None else clearance
        finite = np.sort(among[np.isfinite(among) & (among > -1.0)])
        minimum = float(finite[int(0.3 * (len(finite) - 1))])
    want = self_ref.reduce_pairs(tree, xyzr, link, pairs, poses, fk_status, clearance, e, dist, minimum, flag)
    for a in [xyzr, link, pairs, q, base, poses, fk_status] + [w for w in want if w is not None] + \
            ([limits] if limits is not None else []):
        a.setflags(write=False)
    return Case(names()[index], tree, xyzr, link, pairs, q, minimum, flag, base, limits, poses, fk_status, planted, want)


Coverage = collections.namedtuple(
    "Coverage", "below above equal negative without_value tied_minimum coincident_minimum regular_minimum")


def coverage(index):
    """Counts over the case: pairs below, above and equal to minimum_clearance, negative, without a value; the
    configurations whose minimum is attained by two distinct p (and min_pair is the lower), whose minimum has coincident
    centres (NaN direction and NaN in the gradient), and whose minimum has a finite direction."""
    c = case(index)
    want = c.want
    if want.pair_clearance is None:
        return Coverage(*([0] * 8))
    d = want.pair_clearance
    with np.errstate(invalid="ignore"):
        below = int((d < c.minimum_clearance).sum())
        above = int((d > c.minimum_clearance).sum())
        equal = int((d == c.minimum_clearance).sum())
        negative = int((d < 0.0).sum())
        tied = coincident = regular = 0
        for i in range(len(d)):
            p = int(want.min_pair[i])
            if p < 0:
                continue
            same = np.flatnonzero(d[i] == d[i, p])
            assert same[0] == p
            tied += len(same) > 1
            if np.isnan(want.min_direction[i]).all():
                assert d[i, p] == -(c.xyzr[c.pairs[p, 0], 3] + c.xyzr[c.pairs[p, 1], 3])      # dist == 0
                coincident += 1
            elif np.isfinite(want.min_direction[i]).all():
                regular += 1
    return Coverage(below, above, equal, negative, int(np.isnan(d).sum()), tied, coincident, regular)
