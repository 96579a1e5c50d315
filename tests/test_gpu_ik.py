"""(gpu) vgt_hip_solve_ik[_dev] against tests/ik_ref.py, the CPU restatement: every output bit-equal (NaNs by position) on
the shared cases of tests/ik_cases.py -- through the host form of the product library, the device form on torch buffers,
and the testing library limited to two workgroups, so that 257 problems make the persistent waves stride.  Then the
aliased output, the optional outputs, the argument errors, the forward kinematics of the returned rows (the check that
does not go through new code) and the launch geometry."""
import numpy as np
import pytest

import ik_cases as C
import ik_ref
import kinematics_ref as R
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu

FIELDS = capi.IkSolutions._fields


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def testing():
    """A context of the testing library; its kinematics launches have at most two workgroups unless a test says else."""
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


def assert_equal(got, want, name):
    for field in FIELDS:
        assert same_bits(getattr(got, field), getattr(want, field)), (name, field)


def report(case, got):
    print(case.name, "statuses", np.bincount(got.status, minlength=4).tolist(), "steps: median",
          float(np.median(got.iterations)), "most", int(got.iterations.max()))


def solve_host(context, tree, case):
    return context.solve_ik(tree, case.tip, case.targets, case.seeds, case.seeds_per_target, case.world_from_base,
                            case.joint_limits, **case.options)


GUARD = 16


def solve_dev(context, tree, case, alias=False, without=None):
    """The device form on torch buffers with GUARD sentinels behind each -> IkSolutions; an output named by `without` is
    passed as NULL (its entry is the untouched buffer); alias: joints_out is the seed buffer."""
    import torch
    b, joints = len(case.seeds), case.tree.num_joints
    targets = torch.from_numpy(np.array(case.targets)).cuda()           # (copies: the cases' arrays are read-only)
    seeds = torch.full((b * joints + GUARD,), 77.0, dtype=torch.float64, device="cuda")
    seeds[:b * joints] = torch.from_numpy(np.array(case.seeds).reshape(-1)).cuda()
    sizes = dict(joints=(b * joints, torch.float64), status=(b, torch.uint8), iterations=(b, torch.int32),
                 error=(b * 6, torch.float64), tip_pose=(b * 16, torch.float64), fk_status=(b, torch.uint8))
    out = {f: torch.full((n + GUARD,), 77, dtype=dtype, device="cuda") for f, (n, dtype) in sizes.items()}
    if alias:
        out["joints"] = seeds
    workspace = torch.full((b * joints + GUARD,), 77.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    pointers = {f + "_ptr" if f != "joints" else "joints_out_ptr": (None if f == without else out[f].data_ptr())
                for f in FIELDS if f != "status"}
    context.solve_ik_dev(tree, case.tip, targets.data_ptr(), len(case.targets), seeds.data_ptr(),
                         None if without == "status" else out["status"].data_ptr(), workspace_ptr=workspace.data_ptr(),
                         workspace_bytes=capi.solve_ik_workspace_bytes(joints, b), seeds_per_target=case.seeds_per_target,
                         world_from_base=case.world_from_base, joint_limits=case.joint_limits, **pointers, **case.options)
    context.synchronize()
    host = {f: out[f].cpu().numpy() for f in FIELDS}
    for f, (n, _) in sizes.items():
        assert (host[f][n:] == 77).all(), f
    assert (workspace.cpu().numpy()[b * joints:] == 77.0).all()
    if not alias:
        assert same_bits(seeds.cpu().numpy()[:b * joints].reshape(b, joints), case.seeds)
    shapes = dict(joints=(b, joints), status=(b,), iterations=(b,), error=(b, 6), tip_pose=(b, 16), fk_status=(b,))
    return capi.IkSolutions(*[host[f][:sizes[f][0]].reshape(shapes[f]) for f in FIELDS])


@pytest.mark.parametrize("name", C.case_names())
def test_host_form(ctx, name):
    case = C.case(name)
    with make_tree(ctx, case.tree) as tree:
        got = solve_host(ctx, tree, case)
    report(case, got)
    assert_equal(got, case.want, name)


@pytest.mark.parametrize("name", C.case_names())
def test_device_form(ctx, name):
    case = C.case(name)
    with make_tree(ctx, case.tree) as tree:
        got = solve_dev(ctx, tree, case)
    assert_equal(got, case.want, name)


@pytest.mark.parametrize("name", [n for n in C.case_names() if n.endswith("B257")])
def test_device_form_with_striding_waves(testing, name):
    case = C.case(name)
    with make_tree(testing, case.tree) as tree:
        got = solve_dev(testing, tree, case)
    assert_equal(got, case.want, name)


def test_launch_geometry_does_not_change_a_bit(testing):
    """The same 257 problems under one workgroup and under the launcher's own number of them."""
    case = C.case("arm-1.0-B257")
    with make_tree(testing, case.tree) as tree:
        try:
            testing.set_kinematics_workgroups(1)
            one = solve_dev(testing, tree, case)
            testing.set_kinematics_workgroups(0)
            free = solve_dev(testing, tree, case)
        finally:
            testing.set_kinematics_workgroups(2)
    assert_equal(one, free, "one workgroup against the default")
    assert_equal(one, case.want, "one workgroup")


@pytest.mark.parametrize("name", ["arm-1.0-B257", "body13-weights-R3-B63"])
def test_joints_out_may_be_the_seeds(ctx, name):
    case = C.case(name)
    with make_tree(ctx, case.tree) as tree:
        got = solve_dev(ctx, tree, case, alias=True)
    assert_equal(got, case.want, name)


@pytest.mark.parametrize("without", [f for f in FIELDS if f != "status"])
def test_optional_outputs(ctx, without):
    """Each optional output NULL in turn: its buffer keeps its sentinels, every other output is the answer (without
    joints_out the working rows are the workspace's)."""
    case = C.case("body13-near-B257")
    with make_tree(ctx, case.tree) as tree:
        got = solve_dev(ctx, tree, case, without=without)
    for field in FIELDS:
        if field == without:
            assert (getattr(got, field) == 77).all()
        else:
            assert same_bits(getattr(got, field), getattr(case.want, field)), field


def test_forward_kinematics_of_the_rows_reproduces_the_tip(ctx):
    """vgt_hip_forward_kinematics on joints_out gives tip_pose bit for bit, fk_status is its status on the chain's
    links, and the converged rows are within the tolerances of their targets by that pose."""
    for name in ("arm-1.0-B257", "body13-near-B257", "body8-0.3-B65", "serial-longest-B65"):
        case = C.case(name)
        with make_tree(ctx, case.tree) as tree:
            got = solve_host(ctx, tree, case)
            poses, status = ctx.forward_kinematics(tree, got.joints, case.world_from_base, case.joint_limits)
        # (a NaN in a column off the chain spoils other links, not the tip)
        assert same_bits(poses[:, case.tip], got.tip_pose), name
        assert np.array_equal(status & R.OUTSIDE_LIMITS, got.fk_status & R.OUTSIDE_LIMITS)
        assert ((status & R.NOT_COMPUTABLE) >= (got.fk_status & R.NOT_COMPUTABLE)).all()
        done = got.status == capi.IK_CONVERGED
        aim = np.repeat(case.targets, case.seeds_per_target, axis=0)
        assert done.any() and np.abs(aim[done, 12:15] - poses[done, case.tip, 12:15]).max() <= 1e-6


def test_argument_errors_leave_the_outputs_untouched(ctx):
    """Through the C ABI itself, both forms: each is VGT_HIP_ERR_INVALID_ARGUMENT with its message before any device
    work -- the arrays behind the pointers are small host arrays that no rejected call may touch."""
    lib = ctx._lib
    t = C.tree("arm")
    targets, seeds = np.tile(np.eye(4).reshape(16), (2, 1)), np.zeros((6, t.num_joints))
    outputs = [np.full((6, t.num_joints), 9.0), np.full(6, 9, np.uint8), np.full(6, 9, np.int32), np.full((6, 6), 9.0),
               np.full((6, 16), 9.0), np.full(6, 9, np.uint8)]
    limit = capi.ik_max_chain_joints()
    assert limit >= 16
    mimic = R.Tree([-1, 0, 1], [R.REVOLUTE, R.FIXED, R.PRISMATIC], [0, 0, 0], np.eye(3),
                   np.tile(np.eye(4).reshape(16), (3, 1)), 1)
    long = C.tree("serial-%d" % (limit + 1))
    other = capi.Context(0)
    with make_tree(ctx, t) as tree, make_tree(other, t) as foreign, make_tree(ctx, mimic) as shared, \
            make_tree(ctx, long) as too_long:
        for host in (True, False):
            def refused(needle, context=ctx.handle, tree=tree, tip=7, aim=targets, num_targets=2, per_target=3,
                        start=seeds, weights=None, steps=10, damping=0.01, max_step=0.5, position=1e-6, rotation=1e-6,
                        status=True, joints=True, workspace=(None, 0)):
                out = [capi._ptr(o) for o in outputs]
                arguments = [context, tree._handle_or_raise() if tree else None, tip, capi._ptr(aim), num_targets,
                             per_target, capi._ptr(start), None, None,
                             capi._ptr(None if weights is None else np.array(weights, np.float64)), steps, damping,
                             max_step, position, rotation, out[0] if joints else None, out[1] if status else None,
                             *out[2:]]
                rc = lib.vgt_hip_solve_ik(*arguments) if host else lib.vgt_hip_solve_ik_dev(*arguments, *workspace)
                message = lib.vgt_hip_last_error()
                assert rc == 1 and needle in message, (host, rc, message)

            refused(b"null", context=None)
            refused(b"null", tree=None)
            refused(b"null", aim=None)
            refused(b"null", start=None)
            refused(b"null", status=False)
            refused(b"at least one target", num_targets=0)
            refused(b"at least one target", per_target=0)
            refused(b"at least one target", num_targets=-1)
            refused(b"2^31", num_targets=2 ** 20, per_target=2 ** 11)
            refused(b"tip link -1", tip=-1)
            refused(b"tip link 8", tip=8)
            refused(b"another context", tree=foreign)
            refused(b"max_iterations", steps=-1)
            refused(b"max_iterations", steps=10001)
            refused(b"damping", damping=-1.0)
            refused(b"damping", damping=float("nan"))
            refused(b"damping", damping=float("inf"))
            refused(b"max_step", max_step=0.0)
            refused(b"max_step", max_step=float("nan"))
            refused(b"tolerance", position=-1e-9)
            refused(b"tolerance", rotation=float("nan"))
            refused(b"weight", weights=(1, 1, 1, 1, -1, 1))
            refused(b"weight", weights=(1, 1, float("inf"), 1, 1, 1))
            refused(b"weight", weights=(float("nan"), 1, 1, 1, 1, 1))
            refused(b"links 0 and 2 on the chain to link 2 both read column 0", tree=shared, tip=2, start=np.zeros((6, 1)))
            refused(("%d moving links" % (limit + 1)).encode(), tree=too_long, tip=long.num_links - 1,
                    start=np.zeros((6, limit + 1)))
            if not host:
                refused(b"workspace", joints=False)
                refused(b"workspace", joints=False, workspace=(capi._ptr(seeds), 6 * t.num_joints * 8 - 1))
    other.close()
    for o in outputs:
        assert (o == 9).all()
    assert capi.solve_ik_workspace_bytes(7, 6) == 7 * 6 * 8 and capi.solve_ik_workspace_bytes(7, 0) == 0
    assert capi.solve_ik_workspace_bytes(7, 2 ** 31) == 0 and capi.solve_ik_workspace_bytes(-1, 6) == 0


def test_edges_of_the_argument_ranges_are_taken(ctx):
    """An infinite max_step, infinite tolerances (everything converges at the seed unless half a turn away), a mimic
    joint off the chain, the tip on the base, and the one link of a tree without joints."""
    case = C.case("arm-near-B64-base")
    with make_tree(ctx, case.tree) as tree:
        options = dict(case.options, max_step=float("inf"))
        got = ctx.solve_ik(tree, case.tip, case.targets, case.seeds, 1, case.world_from_base, None, **options)
        want = ik_ref.solve_ik(case.tree, case.tip, case.targets, case.seeds, 1, case.world_from_base, None, **options)
        assert_equal(got, want, "max_step inf")
        options = dict(case.options, position_tolerance=float("inf"), rotation_tolerance=float("inf"))
        got = ctx.solve_ik(tree, case.tip, case.targets, case.seeds, 1, case.world_from_base, None, **options)
        want = ik_ref.solve_ik(case.tree, case.tip, case.targets, case.seeds, 1, case.world_from_base, None, **options)
        assert_equal(got, want, "infinite tolerances")
        assert (got.iterations[got.status == capi.IK_CONVERGED] == 0).all() and got.status[1] != capi.IK_CONVERGED
        # tip 0: one moving link
        got = ctx.solve_ik(tree, 0, case.targets, case.seeds, 1, None, None, **case.options)
        want = ik_ref.solve_ik(case.tree, 0, case.targets, case.seeds, 1, None, None, **case.options)
        assert_equal(got, want, "tip 0")
    body = C.tree("body")
    with make_tree(ctx, body) as tree:
        # tip 6: the left hand's first finger; its mimic partner, link 7, is off this chain
        rng = np.random.default_rng(3)
        truth = (rng.random((65, body.num_joints)) - 0.5) * 2.0
        targets = np.ascontiguousarray(R.forward_kinematics(body, truth)[0][:, 6])
        seeds = truth + (rng.random(truth.shape) - 0.5) * 0.2
        got = ctx.solve_ik(tree, 6, targets, seeds, max_iterations=20)
        want = ik_ref.solve_ik(body, 6, targets, seeds, max_iterations=20)
        assert_equal(got, want, "body tip 6")
    fixed = C.tree("fixed1")
    with make_tree(ctx, fixed) as tree:
        targets = np.tile(fixed.origin[0], (3, 1))
        targets[2, 12] += 1.0
        got = ctx.solve_ik(tree, 0, targets, np.zeros((3, 0)), damping=0.5)
        want = ik_ref.solve_ik(fixed, 0, targets, np.zeros((3, 0)), damping=0.5)
        assert_equal(got, want, "no joints")
        assert got.status.tolist() == [capi.IK_CONVERGED, capi.IK_CONVERGED, capi.IK_ITERATION_LIMIT]
