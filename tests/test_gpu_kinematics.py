"""(gpu) vgt_hip_forward_kinematics[_dev] and vgt_hip_clearance_joint_gradient[_dev] against tests/kinematics_ref.py, the
CPU restatement: poses, status and both gradient forms bit-equal (NaNs by position) on the shared cases of
tests/kinematics_cases.py -- through the host forms of the product library, the device forms on torch buffers, and the
testing library limited to two workgroups, so that 257 configurations make the persistent waves stride.  Then the
optional outputs, the consumers on the forward kinematics' own device output, and the chained call -- without a grid
frame, under a grid turned about a general axis, and with the grid's transform but not its rotation."""
import numpy as np
import pytest

import body_cases
import body_ref
import kinematics_cases as C
import kinematics_ref as R
import projection_cases
import volume_ref
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def few_workgroups():
    """A context of the testing library whose kinematics launches have at most two workgroups."""
    c = capi.Context(0, testing=True)
    c.set_kinematics_workgroups(2)
    yield c
    c.set_kinematics_workgroups(0)
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return np.array_equal(nan_a, nan_b) and np.array_equal(a[~nan_a].view(np.uint64), b[~nan_b].view(np.uint64))


def make_tree(context, t):
    return context.kinematics(*t.arrays(), num_joints=t.num_joints)


def fk_dev(context, tree, case, with_status=True, guard=0):
    """The device form on torch buffers -> (poses, status or None, the guard doubles behind the poses)."""
    import torch
    b, links = len(case.joint_values), case.tree.num_links
    q = torch.from_numpy(np.ascontiguousarray(case.joint_values)).cuda()
    poses = torch.full((b * links * 16 + guard,), 77.0, dtype=torch.float64, device="cuda")
    status = torch.full((b,), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    context.forward_kinematics_dev(tree, q.data_ptr(), b, poses.data_ptr(), status.data_ptr() if with_status else None,
                                   world_from_base=case.world_from_base, joint_limits=case.joint_limits)
    context.synchronize()
    flat = poses.cpu().numpy()
    return flat[:b * links * 16].reshape(b, links, 16), status.cpu().numpy(), flat[b * links * 16:]


def report(case, poses, status):
    print(case.name, "NaN links", int(np.isnan(poses[:, :, 0]).sum()), "statuses", np.bincount(status, minlength=4).tolist())


@pytest.mark.parametrize("index", range(len(C.all_cases())), ids=C.case_names())
def test_forward_kinematics_host_form(ctx, index):
    case = C.case(index)
    with make_tree(ctx, case.tree) as tree:
        assert (tree.num_links, tree.num_joints) == (case.tree.num_links, case.tree.num_joints)
        poses, status = ctx.forward_kinematics(tree, case.joint_values, case.world_from_base, case.joint_limits)
    report(case, poses, status)
    assert same_bits(status, case.status)
    assert same_bits(poses, case.poses)


@pytest.mark.parametrize("index", range(len(C.all_cases())), ids=C.case_names())
def test_forward_kinematics_device_form_with_striding_waves(few_workgroups, index):
    case = C.case(index)
    with make_tree(few_workgroups, case.tree) as tree:
        poses, status, _ = fk_dev(few_workgroups, tree, case)
    report(case, poses, status)
    assert same_bits(status, case.status)
    assert same_bits(poses, case.poses)


def test_forward_kinematics_device_form_of_the_product_library(ctx):
    for index in (4, 9, 14, len(C.all_cases()) - 5):
        case = C.case(index)
        with make_tree(ctx, case.tree) as tree:
            poses, status, _ = fk_dev(ctx, tree, case)
        assert same_bits(status, case.status) and same_bits(poses, case.poses), case.name


def test_one_tree_serves_many_calls_and_options(ctx):
    """One handle, calls with and without base and limits in turn (the limits are uploaded per call)."""
    t = C.tree("body")
    q = C.joint_values(65, t.num_joints, 41)
    with make_tree(ctx, t) as tree:
        for base, limits in ((None, None), (C.base_transform(), C.limits(t.num_joints)), (None, C.limits(t.num_joints)),
                             (C.base_transform().reshape(4, 4).T, None), (None, None)):
            poses, status = ctx.forward_kinematics(tree, q, base, limits)
            base16 = None if base is None else C.base_transform()
            want_poses, want_status = R.forward_kinematics(t, q, base16, limits)
            assert same_bits(poses, want_poses) and same_bits(status, want_status)


def test_optional_status_and_untouched_memory(ctx):
    """status may be NULL; what lies behind the poses, and a status buffer that was not passed, keep their sentinels."""
    case = C.case(9)                                       # arm, B = 257
    with make_tree(ctx, case.tree) as tree:
        poses, status, guard = fk_dev(ctx, tree, case, with_status=False, guard=64)
    assert same_bits(poses, case.poses)
    assert (status == 77).all() and (guard == 77.0).all()


def gradient_dev(context, tree, case, worst, guard=16):
    import torch
    b, s = len(case.poses), len(case.link)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (case.poses, case.xyzr, case.link)]
    pair = (case.min_sphere, case.min_gradient) if worst else (case.weight, case.gradient)
    pair = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in pair]
    count = b * case.tree.num_joints
    out = torch.full((count + guard,), 77.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    names = ("min_sphere_ptr", "min_gradient_ptr") if worst else ("sphere_weight_ptr", "sphere_gradient_ptr")
    context.clearance_joint_gradient_dev(tree, dev[0].data_ptr(), b, dev[1].data_ptr(), dev[2].data_ptr(), s,
                                         out.data_ptr(), **{n: t.data_ptr() for n, t in zip(names, pair)})
    context.synchronize()
    flat = out.cpu().numpy()
    assert (flat[count:] == 77.0).all()
    return flat[:count].reshape(b, case.tree.num_joints)


@pytest.mark.parametrize("index", range(len(C.gradient_case_names())), ids=C.gradient_case_names())
def test_joint_gradient_host_forms(ctx, index):
    case = C.gradient_case(index)
    with make_tree(ctx, case.tree) as tree:
        worst = ctx.clearance_joint_gradient(tree, case.poses, case.xyzr, case.link, min_sphere=case.min_sphere,
                                             min_gradient=case.min_gradient)
        summed = ctx.clearance_joint_gradient(tree, case.poses, case.xyzr, case.link, sphere_weight=case.weight,
                                              sphere_gradient=case.gradient)
    print(case.name, "NaN rows", int(np.isnan(worst).any(axis=1).sum()), int(np.isnan(summed).any(axis=1).sum()))
    assert same_bits(worst, case.want_worst)
    assert same_bits(summed, case.want_summed)


@pytest.mark.parametrize("index", range(len(C.gradient_case_names())), ids=C.gradient_case_names())
def test_joint_gradient_device_forms_with_striding_waves(few_workgroups, index):
    case = C.gradient_case(index)
    with make_tree(few_workgroups, case.tree) as tree:
        assert same_bits(gradient_dev(few_workgroups, tree, case, True), case.want_worst)
        assert same_bits(gradient_dev(few_workgroups, tree, case, False), case.want_summed)


def test_joint_gradient_device_forms_of_the_product_library(ctx):
    case = C.gradient_case(5)
    with make_tree(ctx, case.tree) as tree:
        assert same_bits(gradient_dev(ctx, tree, case, True), case.want_worst)
        assert same_bits(gradient_dev(ctx, tree, case, False), case.want_summed)


def _scene():
    """The arm in the middle of tests/body_cases.py's grid: (tree, joint values [67, 7], base, model)."""
    t = C.tree("arm")
    q = C.joint_values(67, t.num_joints, 77)
    base = np.eye(4)
    base[:3, 3] = [1.5, 1.25, 1.0]
    xyzr, link = C.sphere_model(t, 21, 31)
    return t, q, base.T.reshape(16).copy(), xyzr, link


def test_consumers_take_the_device_output_as_it_stands(ctx):
    """forward_kinematics_dev -> check_spheres_dev and rasterize_spheres_dev on the same device buffer, against
    body_ref / volume_ref on the restated poses."""
    import torch
    from oracle import oracle as O
    t, q, base, xyzr, link = _scene()
    sdf = body_cases.field(False)
    want_poses, _ = R.forward_kinematics(t, q, base)
    want = body_ref.check_spheres(O, sdf, body_cases.RESOLUTION, xyzr, link, want_poses, 0.05)
    want_cells = volume_ref.rasterize_spheres(sdf.shape, body_cases.RESOLUTION, xyzr, link, want_poses, padding=0.02)
    b, s = len(q), len(xyzr)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (q, sdf, xyzr, link)]
    poses = torch.empty((b, t.num_links, 16), dtype=torch.float64, device="cuda")
    shapes = (((b,), torch.uint8), ((b,), torch.float64), ((b,), torch.int32), ((b,), torch.int32), ((b,), torch.int32),
              ((b, 3), torch.float64), ((b, s), torch.float64), ((b, s, 3), torch.float64))
    out = [torch.full(shape, 77, dtype=dtype, device="cuda") for shape, dtype in shapes]
    cells = torch.full(sdf.shape, 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with make_tree(ctx, t) as tree:
        ctx.forward_kinematics_dev(tree, dev[0].data_ptr(), b, poses.data_ptr(), world_from_base=base)
        ctx.check_spheres_dev(dev[1].data_ptr(), sdf.shape, body_cases.RESOLUTION, dev[2].data_ptr(), dev[3].data_ptr(), s,
                              poses.data_ptr(), t.num_links, b, *[a.data_ptr() for a in out], minimum_clearance=0.05)
        ctx.rasterize_spheres_dev(sdf.shape, body_cases.RESOLUTION, dev[2].data_ptr(), dev[3].data_ptr(), s,
                                  poses.data_ptr(), t.num_links, b, cells.data_ptr(), padding=0.02)
        ctx.synchronize()
    got = body_ref.SphereChecks(*[a.cpu().numpy() for a in out])
    print("statuses", np.bincount(got.status, minlength=3).tolist(), "covered cells", int((want_cells >= 0).sum()))
    assert len(set(got.status.tolist())) > 1 and (want_cells >= 0).any()
    for name in body_ref.SphereChecks._fields:
        assert same_bits(getattr(got, name), getattr(want, name)), name
    assert same_bits(cells.cpu().numpy(), want_cells)


def chained_call(ctx, per_sphere, frame):
    """check_spheres_from_joints against forward_kinematics, check_spheres and clearance_joint_gradient in turn; frame:
    (grid_from_world, rotation, world_from_grid) of the grid's origin, the arm's base moved with it, or None."""
    t, q, base, xyzr, link = _scene()
    sdf = body_cases.field(True)
    limits = C.limits(t.num_joints)
    grid_from_world = rotation = None
    if frame is not None:
        grid_from_world, rotation, world_from_grid = frame
        base = projection_cases.base_under(world_from_grid, base)
    grid = dict(grid_from_world=grid_from_world, rotation=rotation)
    with make_tree(ctx, t) as tree:
        got = ctx.check_spheres_from_joints(sdf, body_cases.RESOLUTION, xyzr, link, tree, q, minimum_clearance=0.05,
                                            outside_is_collision=True, per_sphere=per_sphere, world_from_base=base,
                                            joint_limits=limits, joint_gradient=True, **grid)
        poses, fk_status = ctx.forward_kinematics(tree, q, base, limits)
        checks = ctx.check_spheres(sdf, body_cases.RESOLUTION, xyzr, link, poses, 0.05, True, per_sphere=per_sphere, **grid)
        gradient = ctx.clearance_joint_gradient(tree, poses, xyzr, link, min_sphere=checks.min_sphere,
                                                min_gradient=checks.min_gradient)
        plain = ctx.check_spheres_from_joints(sdf, body_cases.RESOLUTION, xyzr, link, tree, q, minimum_clearance=0.05,
                                              outside_is_collision=True, world_from_base=base, **grid)
        none = ctx.check_spheres_from_joints(sdf, body_cases.RESOLUTION, xyzr, link, tree, q[:0], joint_gradient=True)
    for name in capi.SphereChecks._fields:
        g, w = getattr(got, name), getattr(checks, name)
        assert (g is None and w is None) or same_bits(g, w), name
    assert same_bits(got.fk_status, fk_status) and same_bits(got.joint_gradient, gradient)
    assert np.isfinite(gradient).any() and fk_status.any()
    assert plain.joint_gradient is None and plain.sphere_clearance is None and same_bits(plain.status, checks.status)
    assert plain.fk_status.tolist() == (fk_status & 1).tolist()
    assert none.status.shape == (0,) and none.fk_status.shape == (0,) and none.joint_gradient.shape == (0, t.num_joints)
    return got


@pytest.mark.parametrize("per_sphere", [False, True])
def test_chained_call_equals_the_two_steps(ctx, per_sphere):
    chained_call(ctx, per_sphere, None)


@pytest.mark.parametrize("per_sphere", [False, True])
def test_chained_call_under_a_turned_grid(ctx, per_sphere):
    """The same under tests/projection_cases.general_frame_pair(), and directly against the two restatements under the
    frame: every output of the check bit-equal, the joint gradient the restatement's worst-sphere form."""
    from oracle import oracle as O
    frame = projection_cases.general_frame_pair()
    got = chained_call(ctx, per_sphere, frame)
    t, q, base, xyzr, link = _scene()
    base = projection_cases.base_under(frame[2], base)
    want_poses, want_status = R.forward_kinematics(t, q, base, C.limits(t.num_joints))
    want = body_ref.check_spheres(O, body_cases.field(True), body_cases.RESOLUTION, xyzr, link, want_poses, 0.05, True,
                                  frame[0], frame[1])
    for name in capi.SphereChecks._fields:
        if per_sphere or not name.startswith("sphere_"):
            assert same_bits(getattr(got, name), getattr(want, name)), name
    assert same_bits(got.fk_status, want_status)
    assert same_bits(got.joint_gradient, R.clearance_joint_gradient(t, want_poses, xyzr, link, min_sphere=want.min_sphere,
                                                                    min_gradient=want.min_gradient))
    print("statuses", np.bincount(got.status, minlength=3).tolist(), "finite gradient rows",
          int(np.isfinite(got.min_gradient).all(axis=1).sum()))
    assert len(set(got.status.tolist())) > 1 and np.isfinite(got.min_gradient).all(axis=1).any()


def test_the_two_frame_arguments_are_not_interchangeable(ctx):
    """grid_from_world of the frame and no rotation: the same cells, so clearances, statuses, counts and indices are those
    under the frame bit for bit, and the gradients stay in the grid's frame -- those under the frame turned back
    (g * rotation for a row vector g), within 1e-12: another order of operations, so not bit for bit."""
    t, q, base, xyzr, link = _scene()
    grid_from_world, rotation, world_from_grid = projection_cases.general_frame_pair()
    base = projection_cases.base_under(world_from_grid, base)
    sdf = body_cases.field(True)
    r = rotation.reshape(3, 3)
    with make_tree(ctx, t) as tree:
        both, one = [ctx.check_spheres_from_joints(sdf, body_cases.RESOLUTION, xyzr, link, tree, q, minimum_clearance=0.05,
                                                   outside_is_collision=True, per_sphere=True, world_from_base=base,
                                                   grid_from_world=grid_from_world, rotation=turn)
                     for turn in (rotation, None)]
    for name in ("status", "min_clearance", "min_sphere", "num_below", "num_outside", "sphere_clearance", "fk_status"):
        assert same_bits(getattr(one, name), getattr(both, name)), name
    for name in ("min_gradient", "sphere_gradient"):
        g = getattr(both, name)
        with np.errstate(invalid="ignore", over="ignore"):
            back = np.stack([(g[..., 0] * r[0, i] + g[..., 1] * r[1, i]) + g[..., 2] * r[2, i] for i in range(3)], axis=-1)
        # (a gradient with an infinite component is infinite in all three under the frame, and turning it back adds
        # infinities of both signs: only what is finite on both sides has a value to compare)
        finite = np.isfinite(back) & np.isfinite(getattr(one, name))
        worst = float(np.abs(getattr(one, name)[finite] - back[finite]).max())
        moved = float(np.abs(getattr(one, name)[finite] - g[finite]).max())
        print(name, "finite entries", int(finite.sum()), "of", finite.size, "largest difference", worst,
              "and from the turned gradients", moved)
        assert finite.sum() * 2 > finite.size and worst <= 1e-12 and moved > 1e-3
