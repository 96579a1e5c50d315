"""(not gpu) tests/cost_ref.py, the restatement vgt_hip_clearance_cost is compared against: the hinge at its edges, its
continuity and w = dc/dd; the composition -- spheres without a weight are skipped, the NaN-gradient rule and its count,
a model without spheres; the restatement under a turned grid against itself without one; and the coverage of
tests/cost_cases.py, so that no case passes by hitting nothing."""
import numpy as np
import pytest

import cost_cases as C
import cost_ref as R
import kinematics_cases
import kinematics_ref

EPS = 0.25


def bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def test_hinge_values_at_the_edges():
    after = np.nextafter(EPS, np.inf)
    d = np.array([-1.0, -0.0, 0.0, EPS / 2, EPS, after, np.inf, -np.inf, np.nan])
    c, w = R.hinge(d, EPS)
    # d < 0: (eps * 0.5) - d, w = -1
    assert c[0] == 0.125 + 1.0 and w[0] == -1.0
    # -0.0 < 0 is false: the second branch, t = -0.0 - eps = -eps
    for k in (1, 2):
        assert c[k] == ((EPS * EPS) * 0.5) / EPS and w[k] == -EPS / EPS == -1.0
    assert c[3] == ((0.125 * 0.125) * 0.5) / EPS and w[3] == -0.125 / EPS
    # d == eps: t = +0.0, the cost and the weight are +0.0
    assert bits(c[4]) == 0 and bits(w[4]) == 0
    assert bits(c[5]) == 0 and bits(w[5]) == 0 and bits(c[6]) == 0 and bits(w[6]) == 0
    assert c[7] == np.inf and w[7] == -1.0
    assert np.isnan(c[8]) and w[8] == 0.0


@pytest.mark.parametrize("eps", [EPS, 2.0 ** -30, 1000.0, 0.1, 0.3])
def test_hinge_is_continuous_within_one_ulp(eps):
    """c and w on both sides of 0 and of eps: neighbours in d give values within 1 ulp of the limit."""
    zero = np.array([np.nextafter(0.0, -1.0), 0.0])
    c, w = R.hinge(zero, eps)
    assert abs(c[0] - c[1]) <= np.spacing(c[1]) and abs(w[0] - w[1]) <= np.spacing(1.0)
    edge = np.array([np.nextafter(eps, 0.0), eps, np.nextafter(eps, np.inf)])
    c, w = R.hinge(edge, eps)
    assert (c <= np.spacing(0.0) + np.spacing(eps) ** 2 / eps).all() and c[1] == 0.0 and c[2] == 0.0
    assert abs(w[0]) <= np.spacing(1.0) and w[1] == 0.0 and w[2] == 0.0


@pytest.mark.parametrize("eps", [EPS, 0.1, 1000.0])
def test_w_is_the_derivative_of_c(eps):
    """A central difference on the hinge alone, away from the two kinks by more than the step."""
    h = eps * 2.0 ** -20
    d = np.concatenate([np.linspace(-2.0 * eps, -4.0 * h, 50), np.linspace(4.0 * h, eps - 4.0 * h, 50),
                        np.linspace(eps + 4.0 * h, 3.0 * eps, 20)])
    _, w = R.hinge(d, eps)
    up, _ = R.hinge(d + h, eps)
    down, _ = R.hinge(d - h, eps)
    slope = (up - down) / (2.0 * h)
    # c is at most quadratic: the central difference is exact up to the rounding of c, ~eps * 2^-52 / h = 2^-32
    assert np.abs(slope - w).max() <= 2.0 ** -28


def _two_link_tree():
    F, V = kinematics_ref.FIXED, kinematics_ref.REVOLUTE
    origin = np.eye(4)
    origin[:3, 3] = [0.5, 0.0, 0.0]
    return kinematics_ref.Tree([-1, 0], [V, V], [0, 1], [[0, 0, 1], [0, 1, 0]], [np.eye(4).reshape(16), origin.T.reshape(16)], 2)


def _made_up(tree, clearance, gradient, margin):
    q = np.array([[0.3, -0.2]])
    poses, status = kinematics_ref.forward_kinematics(tree, q, None, None)
    clearance = np.asarray(clearance, dtype=np.float64).reshape(1, -1)
    gradient = np.asarray(gradient, dtype=np.float64).reshape(1, -1, 3)
    c, w = R.hinge(clearance, margin)
    return R.Spheres(poses, status, clearance, gradient, c, w)


def test_composition_skips_spheres_without_weight_and_counts():
    tree = _two_link_tree()
    xyzr = np.array([[0.1, 0.0, 0.0, 0.05], [0.0, 0.2, 0.0, 0.05], [0.0, 0.0, 0.3, 0.05], [0.2, 0.1, 0.0, 0.05],
                     [0.1, 0.1, 0.1, 0.05]])
    link = np.array([1, 0, 1, 1, 0], np.int32)
    g = [[1.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, np.nan, 1.0], [0.0, 0.0, 1.0]]
    #   inside, beyond (w 0: its NaN gradient does no harm), below, inside with a NaN gradient, without a value
    d = [0.125, 0.5, -0.25, 0.0625, np.nan]
    per_sphere = _made_up(tree, d, g, EPS)
    got = R.reduce_spheres(tree, xyzr, link, per_sphere)
    assert got.num_active.tolist() == [3] and got.num_outside.tolist() == [1]
    assert got.num_without_gradient.tolist() == [1]
    c = per_sphere.c[0]
    assert got.cost[0] == ((np.float64(0.0) + c[0]) + c[1] + c[2]) + c[3] and not np.isnan(got.cost[0])
    # the gradient is the summed form over the spheres 0 and 2 alone
    weight = np.array([[per_sphere.w[0, 0], 0.0, per_sphere.w[0, 2], 0.0, 0.0]])
    want = kinematics_ref.clearance_joint_gradient(tree, per_sphere.poses, xyzr, link, sphere_weight=weight,
                                                   sphere_gradient=per_sphere.gradient)
    assert np.array_equal(bits(got.joint_gradient), bits(want)) and np.isfinite(want).all() and want.any()
    # every sphere beyond the margin: +0.0 everywhere
    per_sphere = _made_up(tree, [0.5] * 5, g, EPS)
    got = R.reduce_spheres(tree, xyzr, link, per_sphere)
    assert bits(got.cost).tolist() == [0] and (bits(got.joint_gradient) == 0).all() and got.num_active.tolist() == [0]


def test_a_model_without_spheres():
    index = C.names().index("arm-0")
    want = C.case(index).want
    assert (bits(want.cost) == 0).all() and (bits(want.joint_gradient) == 0).all()
    assert want.joint_gradient.shape == (C.NUM_CONFIGURATIONS, 7)
    assert not want.num_active.any() and not want.num_outside.any() and not want.num_without_gradient.any()
    assert want.fk_status.any()


def agree(got, want, bound, undefined_rows=None):
    """NaNs and infinities in the same places (the infinities with their signs), everything else within `bound`; -> the
    largest difference.  In the rows of `undefined_rows` (a mask) a value that is not finite is only held to be not
    finite on both sides."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape
    finite = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), finite)
    strict = ~finite
    if undefined_rows is not None:
        strict = strict & ~np.asarray(undefined_rows, dtype=bool).reshape((-1,) + (1,) * (got.ndim - 1))
    assert np.array_equal(np.isnan(got[strict]), np.isnan(want[strict]))
    infinite = strict & ~np.isnan(want)
    assert np.array_equal(got[infinite], want[infinite])
    worst = float(np.abs(got[finite] - want[finite]).max()) if finite.any() else 0.0
    assert worst <= bound, worst
    return worst


@pytest.mark.parametrize("name", ["arm-21", "arm-64-odd", "arm-257-odd", "body-9-odd"])
def test_the_restatement_under_a_turned_grid(name):
    """The restatement under tests/projection_cases.general_frame_pair(), held to itself without a frame: the grid turned
    and shifted and the tree with it (world_from_grid * world_from_base) is the same scene, so every sphere has the same
    cell and the same clearance up to the rounding of two more transforms, its gradient is the plain one turned into the
    world (g * rotation^T for a row vector g), and the joint gradient -- a derivative with respect to the joints --
    does not depend on the frame.  No configuration and no sphere is left out.  A frame applied the wrong way round, or
    a gradient left in the grid's frame, moves these values by 1e-3 or more.

    One thing does depend on the frame, and only on the fields with infinite cells: an active sphere whose gradient has
    an infinite component.  It is no NaN gradient, so it keeps its weight; its terms are then +-infinity, and whether
    their sum is an infinity or a NaN depends on their signs.  Turned, the gradient is infinite in all three components
    (no entry of the rotation is 0), so the signs differ from the plain ones: in body-9-odd 17 joint-gradient entries in
    7 configurations are an infinity on one side and a NaN on the other.  Neither is a value.  In exactly the
    configurations that have such a sphere the joint gradient is therefore held to be finite in the same places and
    within the bound there; everywhere else NaNs and infinities are in the same places too."""
    from oracle import oracle as O
    import projection_cases
    case = C.case(C.names().index(name))
    assert case.grid_from_world is None and case.rotation is None
    grid_from_world, rotation, world_from_grid = projection_cases.general_frame_pair()
    base = projection_cases.base_under(world_from_grid, case.world_from_base)
    turned = R.spheres(O, case.sdf, C.RESOLUTION, case.xyzr, case.link, case.tree, case.joint_values, case.margin,
                       grid_from_world, rotation, base, case.joint_limits)
    got = R.reduce_spheres(case.tree, case.xyzr, case.link, turned)
    want = case.want
    for field in ("num_active", "num_outside", "num_without_gradient", "fk_status"):
        assert np.array_equal(getattr(got, field), getattr(want, field)), field
    g = case.spheres.gradient
    undefined = ((case.spheres.w != 0.0) & np.isinf(g).any(axis=2) & ~np.isnan(g).any(axis=2)).any(axis=1)
    assert not undefined.any() or name.endswith("-odd")
    print(name, "configurations with an active sphere of infinite gradient:", np.flatnonzero(undefined).tolist())
    worst = [agree(got.cost, want.cost, 1e-9), agree(got.joint_gradient, want.joint_gradient, 1e-9, undefined)]
    with np.errstate(invalid="ignore", over="ignore"):
        r = rotation.reshape(3, 3)
        rotated = np.stack([(g[..., 0] * r[i, 0] + g[..., 1] * r[i, 1]) + g[..., 2] * r[i, 2] for i in range(3)], axis=-1)
    worst.append(agree(turned.gradient, rotated, 1e-12))
    worst.append(agree(turned.clearance, case.spheres.clearance, 1e-12))
    print(name, "largest differences: cost %g, joint gradient %g, turned gradients %g, clearances %g" % tuple(worst))
    assert want.num_active.any() and np.isfinite(want.joint_gradient).any() and want.joint_gradient[np.isfinite(want.joint_gradient)].any()


def test_cases_cover_what_they_claim():
    names = C.names()
    assert len(set(names)) == len(names)
    total_outside = total_without_gradient = 0
    for index, (tree, s, odd, b, margin, radius) in enumerate(C.CASES):
        below, inside, beyond, outside, without_gradient, on_edge = C.coverage(index)
        print(names[index], "d<0", below, "0<=d<=eps", inside, "d>eps", beyond, "without a value", outside,
              "active with a NaN gradient", without_gradient, "d==eps", on_edge)
        total_outside += outside
        total_without_gradient += without_gradient
        moving = kinematics_cases.tree(tree).num_joints > 0
        if index in C.FRAMED:
            # the frame cases: all three hinge branches, under a grid_from_world and a rotation that are there
            assert below > 0 and inside > 0 and beyond > 0, names[index]
            framed = C.case(index)
            assert framed.grid_from_world is not None and framed.rotation is not None
            if (tree, s, odd) == ("arm", 65, True):
                assert framed.want.num_without_gradient.sum() > 0 and framed.want.num_outside.sum() > 0
                assert framed.joint_limits is not None and (framed.want.fk_status & 2).any()
        if margin == C.MARGIN and s >= 5 and moving and b == C.NUM_CONFIGURATIONS:
            assert below > 0 and inside > 0 and beyond > 0, names[index]
        if margin == C.EDGE:
            assert on_edge > 0 and C.case(index).margin > 0.0
        want = C.case(index).want
        assert (want.num_without_gradient.sum(), want.num_outside.sum()) == (without_gradient, outside)
    assert total_outside > 0 and total_without_gradient > 0
    # the planted radius: a clearance of exactly +0.0, which takes the second branch
    case = C.case(names.index("arm-21-odd-radius"))
    zero = np.flatnonzero(bits(case.spheres.clearance[3]) == 0)
    assert len(zero) >= 1 and (case.spheres.w[3, zero] == -1.0).all()
    assert (case.spheres.c[3, zero] == ((case.margin * case.margin) * 0.5) / case.margin).all()
    # batch sizes on both sides of the tile
    t = C.tile_samples()
    assert {b for tree, s, odd, b, m, r in C.CASES if (tree, s) == ("arm", 21)} >= {1, t - 1, t, t + 1, 67, 257}
