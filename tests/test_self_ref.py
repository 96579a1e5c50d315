"""(not gpu) tests/self_ref.py, the restatement vgt_hip_check_self_collision is compared against: hand-derived answers on
a two-link tree (clearances, the tie, the coincident pair, the status rules, pairs and links out of range), the gradient
against central differences, and the coverage of tests/self_cases.py, so that no case passes by hitting nothing."""
import numpy as np

import kinematics_cases
import kinematics_ref
import self_cases as C
import self_ref as R


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _two_link_tree():
    V = kinematics_ref.REVOLUTE
    origin = np.eye(4)
    origin[:3, 3] = [0.5, 0.0, 0.0]
    return kinematics_ref.Tree([-1, 0], [V, V], [0, 1], [[0, 0, 1], [0, 0, 1]],
                               [np.eye(4).reshape(16), origin.T.reshape(16)], 2)


def test_hand_derived_answers():
    tree = _two_link_tree()
    # q = 0: link 1 sits at (0.5, 0, 0), unrotated
    xyzr = np.array([[0.0, 0.0, 0.0, 0.125], [0.0, 0.0, 0.0, 0.25], [0.0, 0.0, 0.0, 0.25], [0.5, 0.0, 0.0, 0.0625],
                     [0.0, 0.0, 1.0, 0.0]])
    link = np.array([0, 1, 1, 0, 0], np.int32)
    pairs = np.array([[0, 4], [0, 1], [0, 2], [1, 3], [2, 3], [0, 7], [-1, 2]], np.int32)
    got = R.check_self_collision(xyzr, link, pairs, tree, np.zeros((1, 2)), minimum_clearance=0.125)
    # 1.0 - 0.125 - 0;  0.5 - 0.125 - 0.25 twice;  sphere 3 is where the spheres 1 and 2 are: 0 - 0.25 - 0.0625
    assert got.pair_clearance[0, :5].tolist() == [0.875, 0.125, 0.125, -0.3125, -0.3125]
    assert np.isnan(got.pair_clearance[0, 5:]).all()
    assert got.num_below.tolist() == [4] and got.num_without_value.tolist() == [2]
    assert got.min_pair.tolist() == [3] and got.min_clearance.tolist() == [-0.3125]
    assert got.status.tolist() == [R.COLLISION] and got.fk_status.tolist() == [0]
    assert np.isnan(got.min_direction).all() and np.isnan(got.joint_gradient).all()
    # without the coincident pairs: the tie of the pairs 1 and 2, the direction from b to a
    got = R.check_self_collision(xyzr, link, pairs[:3], tree, np.zeros((1, 2)), minimum_clearance=0.0)
    assert got.min_pair.tolist() == [1] and got.status.tolist() == [R.CLEAR]
    assert got.min_direction.tolist() == [[-1.0, 0.0, 0.0]]
    # turning either joint about z does not change the distance between the origins of the two links
    assert (bits(got.joint_gradient) << np.uint64(1) == 0).all()
    # the status rules: no pair with a value; the flag
    got = R.check_self_collision(xyzr, link, pairs[5:], tree, np.zeros((1, 2)))
    assert got.status.tolist() == [R.NO_VALUE] and got.min_pair.tolist() == [-1] and np.isnan(got.min_clearance).all()
    assert np.isnan(got.joint_gradient).all() and got.num_without_value.tolist() == [2]
    got = R.check_self_collision(xyzr, link, pairs[5:], tree, np.zeros((1, 2)), no_value_is_collision=True)
    assert got.status.tolist() == [R.COLLISION]
    # no pairs, no spheres
    for model in ((xyzr, link, pairs[:0]), (xyzr[:0], link[:0], pairs)):
        got = R.check_self_collision(*model, tree, np.zeros((3, 2)), no_value_is_collision=True)
        assert got.status.tolist() == [R.NO_VALUE] * 3 and got.min_pair.tolist() == [-1] * 3
        assert not got.num_below.any() and not got.num_without_value.any() and np.isnan(got.joint_gradient).all()


def test_gradient_is_the_derivative_of_the_minimum_clearance():
    """Central differences on the arm, in configurations whose worst pair stays the worst."""
    tree = kinematics_cases.tree("arm")
    xyzr, link = kinematics_cases.sphere_model(tree, 12, 3)
    pairs = R.self_collision_pairs(link, tree.num_links)
    rng = np.random.default_rng(1)
    q = rng.random((6, tree.num_joints)) * 2.0 - 1.0
    got = R.check_self_collision(xyzr, link, pairs, tree, q)
    h = 2.0 ** -20
    checked = 0
    for j in range(tree.num_joints):
        step = np.zeros(tree.num_joints)
        step[j] = h
        up = R.check_self_collision(xyzr, link, pairs, tree, q + step)
        down = R.check_self_collision(xyzr, link, pairs, tree, q - step)
        same = (up.min_pair == got.min_pair) & (down.min_pair == got.min_pair)
        slope = (up.min_clearance - down.min_clearance) / (2.0 * h)
        assert np.abs(slope - got.joint_gradient[:, j])[same].max() <= 2.0 ** -18
        checked += int(same.sum())
    assert checked >= 30 and np.abs(got.joint_gradient).max() > 0.01


def test_pair_generator_restatement():
    link = [0, 0, 1, 2, 2]
    assert R.self_collision_pairs(link, 3).tolist() == [[0, 2], [0, 3], [0, 4], [1, 2], [1, 3], [1, 4], [2, 3], [2, 4]]
    assert R.self_collision_pairs(link, 3, parent=[-1, 0, 1], skip_adjacent=True).tolist() == \
        [[0, 3], [0, 4], [1, 3], [1, 4]]
    assert R.self_collision_pairs(link, 3, parent=[-1, 0, 1]).shape == (8, 2)
    assert R.self_collision_pairs(link, 3, ignored_link_pairs=[[2, 0]]).tolist() == [[0, 2], [1, 2], [2, 3], [2, 4]]
    assert R.self_collision_pairs([1, 1, 1], 3).shape == (0, 2)


def test_cases_cover_what_they_claim():
    names = C.names()
    assert len(set(names)) == len(names)
    for index, (tree, s, b, minimum) in enumerate(C.CASES):
        c = C.case(index)
        cover = C.coverage(index)
        print(names[index], "P", len(c.pairs), cover)
        if c.planted is None:
            continue
        # every planted case: below, above and equal to the margin, negative, without a value, a tie for the minimum
        # that went to the lower p, a coincident minimum
        assert cover.below > 0 and cover.above > 0 and cover.negative > 0 and cover.without_value > 0, names[index]
        assert cover.tied_minimum > 0 and cover.coincident_minimum > 0, names[index]
        if minimum == C.EDGE:
            assert cover.equal > 0, names[index]
        if c.tree.num_joints > 0 and b >= 7:
            assert cover.regular_minimum > 0, names[index]
        want = c.want
        if c.tree.num_joints > 0:
            coincident = np.isnan(want.min_direction).all(axis=1) & (want.min_pair >= 0)
            assert np.isnan(want.joint_gradient[coincident]).any(axis=1).all(), names[index]
        assert set(np.unique(want.status).tolist()) <= {R.CLEAR, R.COLLISION, R.NO_VALUE}
    planted = [i for i in range(len(C.CASES)) if C.case(i).planted is not None]
    assert len(planted) >= 10
    # the planted joint rows: a configuration without any value, unless the flag makes it a collision
    arm = C.case(names.index("arm-21"))
    assert arm.want.min_pair[5] == -1 and arm.want.fk_status[5] & 1
    statuses = np.concatenate([C.case(i).want.status for i in range(len(C.CASES))])
    assert {R.CLEAR, R.COLLISION, R.NO_VALUE} <= set(statuses.tolist())
    # batch sizes on both sides of the tile, and trees on both sides of one configuration per tile
    t = C.tile_formula(8, 21)
    assert {b for tree, s, b, m in C.CASES if (tree, s) == ("arm", 21)} >= {1, t - 1, t, t + 1, 67, 257}
    links = int(C.one_per_tile_chain().split("-")[1])
    assert C.tile_formula(links, 21) == 1 and C.tile_formula(links - 1, 21) == 2
    assert C.tile_formula(1, 2037) == 1 and C.tile_formula(1, 2038) == 0 and C.tile_formula(681, 0) == 0
