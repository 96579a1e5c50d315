"""(not gpu) tests/kinematics_ref.py, the restatement the GPU tests hold vgt_hip_forward_kinematics and
vgt_hip_clearance_joint_gradient to, checked on its own: the accuracy of its sin / cos, an independent route to the
poses (4 x 4 matrix products with np.sin / np.cos), central differences for the joint gradient, the status bits and how
far NaN reaches."""
import numpy as np
import pytest

import kinematics_cases as C
import kinematics_ref as R

ULP = 2.0 ** -53


def test_sin_cos_accuracy():
    """Within 4 * 2^-53 absolute of np.sin / np.cos for |q| <= 2^20: twice the worst case measured when the definition
    was written (2 * 2^-53, over 4 * 10^6 uniform samples in each of +-pi, +-100, +-2^16, +-2^20 and multiples of pi / 4);
    the same bound for |s^2 + c^2 - 1|.  The measured worst case is printed."""
    rng = np.random.default_rng(11)
    worst_s = worst_c = worst_unit = 0.0
    samples = [(rng.random(4000000) * 2.0 - 1.0) * span for span in (np.pi, 100.0, 2.0 ** 16, 2.0 ** 20)]
    samples.append(np.arange(-4000, 4001) * (np.pi / 4))
    samples.append(np.array([2.0 ** 20, -2.0 ** 20, np.nextafter(2.0 ** 20, 0.0), 1e-300, -1e-300, 5e-324]))
    for q in samples:
        s, c = R.sincos(q)
        worst_s = max(worst_s, float(np.abs(s - np.sin(q)).max()))
        worst_c = max(worst_c, float(np.abs(c - np.cos(q)).max()))
        worst_unit = max(worst_unit, float(np.abs(s * s + c * c - 1.0).max()))
    print("worst |sin - np.sin| = %.3g ulp(1/2), |cos - np.cos| = %.3g, |s^2 + c^2 - 1| = %.3g (units of 2^-53)"
          % (worst_s / ULP, worst_c / ULP, worst_unit / ULP))
    assert worst_s <= 4 * ULP and worst_c <= 4 * ULP and worst_unit <= 4 * ULP


def test_zero_gives_exactly_zero_and_one():
    s, c = R.sincos(np.array([0.0, -0.0]))
    assert s[0] == 0.0 and not np.signbit(s[0]) and c.tolist() == [1.0, 1.0] and s[1] == 0.0
    # ... so a zero joint leaves the pose untouched bit for bit
    tree = C.tree("arm")
    poses, status = R.forward_kinematics(tree, np.zeros((1, 7)))
    fixed = R.Tree(tree.parent, np.zeros(8, np.int32), tree.joint_index, tree.axis, tree.origin, 7)
    want, _ = R.forward_kinematics(fixed, np.zeros((1, 7)))
    assert np.array_equal(poses.view(np.uint64), want.view(np.uint64)) and status.tolist() == [0]


def _independent(tree, q, base):
    """[L, 4, 4] by matrix products with numpy's own sin / cos and Rodrigues' formula on the unit axis"""
    out = np.zeros((tree.num_links, 4, 4))
    for i in range(tree.num_links):
        origin = tree.origin[i].reshape(4, 4).T.copy()
        origin[3] = [0, 0, 0, 1]
        parent = tree.parent[i]
        above = out[parent] if parent >= 0 else (np.eye(4) if base is None else base)
        joint = np.eye(4)
        if tree.joint_type[i] == R.REVOLUTE:
            a, v = tree.axis[i], q[tree.joint_index[i]]
            k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
            # (the header's rotation for an axis of any length: cos I + (1 - cos) a a^T + sin [a]x)
            joint[:3, :3] = np.cos(v) * np.eye(3) + (1 - np.cos(v)) * np.outer(a, a) + np.sin(v) * k
        elif tree.joint_type[i] == R.PRISMATIC:
            joint[:3, 3] = tree.axis[i] * q[tree.joint_index[i]]
        out[i] = above @ origin @ joint
    return out


@pytest.mark.parametrize("name", ["fixed1", "arm", "body"])
def test_independent_route(name):
    """Within 1e-12 * (1 + max |translation|) for depth <= 8: a few 1e-16 relative per level, times the depth, times a
    margin of 100."""
    tree = C.tree(name)
    rng = np.random.default_rng(3)
    q = (rng.random((40, tree.num_joints)) * 2 - 1) * np.pi
    for base16 in (None, C.base_transform()):
        base = None
        if base16 is not None:
            base = base16.reshape(4, 4).T.copy()
            base[3] = [0, 0, 0, 1]
        poses, status = R.forward_kinematics(tree, q, base16)
        assert not status.any()
        worst = 0.0
        for b in range(len(q)):
            want = _independent(tree, q[b], base)
            got = poses[b].reshape(-1, 4, 4).transpose(0, 2, 1)
            assert np.array_equal(got[:, 3], np.tile([0.0, 0, 0, 1], (tree.num_links, 1)))
            bound = 1e-12 * (1 + np.abs(want[:, :3, 3]).max())
            worst = max(worst, float(np.abs(got - want).max() / bound))
            assert np.abs(got - want).max() <= bound
        print(name, "base" if base is not None else "no base", "worst error / bound = %.3g" % worst)


def test_the_first_link_without_a_base_is_its_origin_as_it_stands():
    tree = C.tree("fixed1")
    poses, _ = R.forward_kinematics(tree, np.zeros((3, 0)))
    want = tree.origin[0].copy()
    want[3::4] = [0, 0, 0, 1]
    assert np.array_equal(poses[:, 0].view(np.uint64), np.tile(want, (3, 1)).view(np.uint64))


@pytest.mark.parametrize("name", ["arm", "body"])
def test_joint_gradient_against_central_differences(name):
    """d (g . p) / d q_j by central differences of the restated forward kinematics, h = 1e-6: within
    1e-7 * (1 + |p|) * |g| (truncation of order h^2, round-off about 1e-10).  The revolute axes are made unit here: with
    an axis of another length the header's R is no rotation and a x d is not its derivative (prismatic axes of any
    length are)."""
    tree = C.tree(name)
    axis = tree.axis.copy()
    revolute = tree.joint_type == R.REVOLUTE
    axis[revolute] /= np.linalg.norm(axis[revolute], axis=1, keepdims=True)
    tree = R.Tree(tree.parent, tree.joint_type, tree.joint_index, axis, tree.origin, tree.num_joints)
    rng = np.random.default_rng(17)
    num = 6
    q = (rng.random((num, tree.num_joints)) * 2 - 1) * 2.0
    xyzr, link = C.sphere_model(tree, 9, 4)
    g = rng.normal(size=(num, 3))
    s = rng.integers(0, len(link), num).astype(np.int32)
    poses, _ = R.forward_kinematics(tree, q)
    got = R.clearance_joint_gradient(tree, poses, xyzr, link, min_sphere=s, min_gradient=g)

    def centres(values):
        p, _ = R.forward_kinematics(tree, values)
        return np.array([R._sphere_centre(p[b, link[s[b]]], xyzr[s[b]]) for b in range(num)])

    h = 1e-6
    worst = 0.0
    for j in range(tree.num_joints):
        step = np.zeros_like(q)
        step[:, j] = h
        up, down = centres(q + step), centres(q - step)
        want = ((up - down) * g).sum(axis=1) / (2 * h)
        bound = 1e-7 * (1 + np.linalg.norm(centres(q), axis=1)) * np.linalg.norm(g, axis=1)
        worst = max(worst, float((np.abs(got[:, j] - want) / bound).max()))
        assert (np.abs(got[:, j] - want) <= bound).all(), j
    print(name, "worst error / bound = %.3g" % worst)


def test_summed_form_with_a_one_hot_weight_is_the_worst_sphere_form():
    tree = C.tree("body")
    rng = np.random.default_rng(23)
    num, count = 12, 7
    q = (rng.random((num, tree.num_joints)) * 2 - 1) * 2.0
    xyzr, link = C.sphere_model(tree, count, 6)
    poses, _ = R.forward_kinematics(tree, q)
    s = rng.integers(0, count, num).astype(np.int32)
    g = rng.normal(size=(num, 3))
    weight = np.zeros((num, count))
    weight[np.arange(num), s] = 1.0
    gradients = np.full((num, count, 3), np.nan)                 # (a sphere of weight 0 is skipped: its NaN does no harm)
    gradients[np.arange(num), s] = g
    worst = R.clearance_joint_gradient(tree, poses, xyzr, link, min_sphere=s, min_gradient=g)
    summed = R.clearance_joint_gradient(tree, poses, xyzr, link, sphere_weight=weight, sphere_gradient=gradients)
    assert np.isfinite(worst).all() and np.array_equal(worst.view(np.uint64), summed.view(np.uint64))
    # outside [0, S), or a link outside [0, L): the row is NaN; the summed form skips such a sphere
    bad_link = link.copy()
    bad_link[s[0]] = tree.num_links
    s2 = s.copy()
    s2[1], s2[2] = -1, count
    got = R.clearance_joint_gradient(tree, poses, xyzr, bad_link, min_sphere=s2, min_gradient=g)
    assert np.isnan(got[:3]).all()
    got = R.clearance_joint_gradient(tree, poses, xyzr, bad_link, sphere_weight=weight, sphere_gradient=gradients)
    assert (got[0] == 0.0).all() and not np.signbit(got[0]).any()


def test_status_bits_and_how_far_nan_reaches():
    tree = C.tree("body")
    q = np.zeros((8, tree.num_joints))
    q[1, 2] = np.nan                 # link 4 (revolute, left arm): 4 and its descendants 5, 6, 7, 8
    q[2, 0] = np.inf                 # link 1 (the prismatic lift): everything above the mount
    q[3, 9] = np.nextafter(2.0 ** 20, np.inf)      # link 14 (the camera): only itself
    q[4, 9] = -2.0 ** 20             # computable
    q[5, 8] = 2.0 ** 30              # a prismatic link takes any finite value
    q[6, 4] = -np.inf                # the mimic column: links 6 and 7
    limits = C.limits(tree.num_joints)
    q[7, 3] = np.nextafter(C.LIMIT, np.inf)
    poses, status = R.forward_kinematics(tree, q, None, limits)
    nan_links = [sorted(set(np.nonzero(np.isnan(poses[b, :, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]]).any(axis=0))[0]))
                 for b in range(8)]
    assert nan_links == [[], [4, 5, 6, 7, 8], list(range(1, 15)), [14], [], [], [6, 7], []]
    for b in range(8):
        for k in nan_links[b]:
            assert np.isnan(poses[b, k, [0, 1, 2, 4, 5, 6, 8, 9, 10, 12, 13, 14]]).all()
    assert np.array_equal(poses[:, :, 3::4], np.tile([0.0, 0, 0, 1], (8, 15, 1)))
    # NaN compares false: no OUTSIDE_LIMITS for it; infinities and 2^20 are outside +-2.5
    assert status.tolist() == [0, 1, 1 | 2, 1 | 2, 2, 2, 1 | 2, 2]
    _, without = R.forward_kinematics(tree, q)
    assert without.tolist() == [0, 1, 1, 1, 0, 0, 1, 0]
    # values on the limits are inside
    on = np.tile(limits[:, 1], (2, 1))
    on[1] = limits[:, 0]
    assert R.forward_kinematics(tree, on, None, limits)[1].tolist() == [0, 0]


def test_shared_cases_have_the_planted_rows():
    statuses = set()
    for index in range(len(C.all_cases())):
        case = C.case(index)
        statuses |= set(case.status.tolist())
        assert case.poses.shape == (len(case.joint_values), case.tree.num_links, 16)
    assert statuses == {0, 1, 2, 3}
