"""(gpu) vgt_hip_clearance_cost[_dev] against tests/cost_ref.py, the CPU restatement: all six outputs bit-equal (NaNs by
position) on the shared cases of tests/cost_cases.py -- through the host form of the product library, and the device
form on torch buffers through the testing library limited to two workgroups, so that 67 configurations make the
persistent waves stride.  Then the cost-only form, the optional outputs, the GPU entry points that exist without this
call (check_spheres_from_joints, a numpy hinge, the summed clearance_joint_gradient), in the device form links outside
the tree and a model without spheres, trees at the kernel's limits, and the argument errors that need a tree.

The cases of cost_cases.FRAMED pass a grid_from_world and a rotation (a turn about a general axis), in both forms; one
test passes the first without the second.  The links the gradient's walk reads are run on both sides of the kernel's
LDS, the shapes chosen by the launcher's own geometry (capi.cost_launch_geometry)."""
import numpy as np
import pytest

import body_cases
import cost_cases as C
import cost_ref as R
import kinematics_cases
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu

FIELDS = capi.ClearanceCosts._fields


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def few_workgroups():
    """A context of the testing library whose cost launches have at most two workgroups."""
    c = capi.Context(0, testing=True)
    c.set_cost_workgroups(2)
    yield c
    c.set_cost_workgroups(0)
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


def assert_same(got, want, what, fields=FIELDS):
    for name in fields:
        g, w = getattr(got, name), getattr(want, name)
        if not same_bits(g, w):
            rows = np.flatnonzero([not same_bits(g[e], w[e]) for e in range(len(w))])
            raise AssertionError("%s: %s differs in configurations %s: got %s, want %s"
                                 % (what, name, rows[:8].tolist(), g[rows[:3]].tolist(), w[rows[:3]].tolist()))


def host_form(context, tree, case, **kw):
    return context.clearance_cost(case.sdf, C.RESOLUTION, case.xyzr, case.link, tree, case.joint_values, case.margin,
                                  grid_from_world=case.grid_from_world, rotation=case.rotation,
                                  world_from_base=case.world_from_base, joint_limits=case.joint_limits, **kw)


GUARD = 16
OUTPUTS = (("cost", "float64"), ("joint_gradient", "float64"), ("num_active", "int32"), ("num_outside", "int32"),
           ("num_without_gradient", "int32"), ("fk_status", "uint8"))


def device_form(context, tree, case, without=(), num_spheres=None):
    """The device form on torch buffers filled with 77, GUARD elements behind each output -> ClearanceCosts; the outputs
    named in `without` are passed as NULL and come back as they were.  Asserts that the guards are untouched."""
    import torch
    num, joints = case.joint_values.shape
    inputs = [case.sdf, case.xyzr, case.link, case.joint_values]
    if joints == 0:
        inputs[3] = np.zeros(1)
    if len(case.link) == 0:                                # (torch has no pointer for an empty tensor: one element stands in)
        inputs[1], inputs[2] = np.zeros((1, 4)), np.zeros(1, np.int32)
    dev = [torch.from_numpy(np.array(a)).cuda() for a in inputs]        # (copies: the cases are read-only)
    widths = {name: joints if name == "joint_gradient" else 1 for name, _ in OUTPUTS}
    out = {name: torch.full((num * widths[name] + GUARD,), 77, dtype=getattr(torch, dtype), device="cuda")
           for name, dtype in OUTPUTS}
    torch.cuda.synchronize()
    pointers = {name + "_ptr": None if name in without else out[name].data_ptr() for name in out if name != "cost"}
    context.clearance_cost_dev(dev[0].data_ptr(), case.sdf.shape, C.RESOLUTION, dev[1].data_ptr(), dev[2].data_ptr(),
                               len(case.link) if num_spheres is None else num_spheres, tree, dev[3].data_ptr(), num,
                               case.margin, out["cost"].data_ptr(), grid_from_world=case.grid_from_world,
                               rotation=case.rotation, world_from_base=case.world_from_base,
                               joint_limits=case.joint_limits, **pointers)
    context.synchronize()
    got = []
    for name, _ in OUTPUTS:
        flat = out[name].cpu().numpy()
        assert (flat[num * widths[name]:] == 77).all(), "the guard behind %s" % name
        flat = flat[:num * widths[name]]
        got.append(flat.reshape(num, joints) if name == "joint_gradient" else flat)
    return capi.ClearanceCosts(*got)


def report(case, got):
    print(case.name, "active", int(got.num_active.sum()), "outside", int(got.num_outside.sum()), "without gradient",
          int(got.num_without_gradient.sum()), "tile", capi.cost_tile_samples(case.tree.num_links))


@pytest.mark.parametrize("index", range(len(C.CASES)), ids=C.names())
def test_host_form(ctx, index):
    case = C.case(index)
    with make_tree(ctx, case.tree) as tree:
        got = host_form(ctx, tree, case)
    report(case, got)
    assert_same(got, case.want, case.name)


@pytest.mark.parametrize("index", range(len(C.CASES)), ids=C.names())
def test_device_form_with_striding_waves(few_workgroups, index):
    case = C.case(index)
    with make_tree(few_workgroups, case.tree) as tree:
        got = device_form(few_workgroups, tree, case)
    report(case, got)
    assert_same(got, case.want, case.name)


COST_ONLY = [name for name in C.names() if name in ("arm-21", "arm-70", "arm-257-odd", "body-9-odd", "arm-0", "fixed1-2",
                                                    "arm-65-odd-frame")]


@pytest.mark.parametrize("name", COST_ONLY)
def test_cost_only_form(ctx, few_workgroups, name):
    """joint_gradient NULL (and with it num_without_gradient, which needs the gradients): the same cost and counts, and
    the gradient buffer untouched."""
    case = C.case(C.names().index(name))
    kept = ("cost", "num_active", "num_outside", "fk_status")
    with make_tree(few_workgroups, case.tree) as tree:
        got = device_form(few_workgroups, tree, case, without=("joint_gradient", "num_without_gradient"))
        counted = device_form(few_workgroups, tree, case, without=("joint_gradient",))
    assert_same(got, case.want, case.name, kept)
    assert (got.joint_gradient == 77).all() and (got.num_without_gradient == 77).all()
    # the count of skipped gradients alone: the gradient kernel without its walk
    assert_same(counted, case.want, case.name, kept + ("num_without_gradient",))
    assert (counted.joint_gradient == 77).all()
    with make_tree(ctx, case.tree) as tree:
        scored = host_form(ctx, tree, case, with_gradient=False)
    assert scored.joint_gradient is None and scored.num_without_gradient is None
    assert_same(scored, case.want, case.name, kept)


def test_device_form_of_the_product_library(ctx):
    case = C.case(C.names().index("body-9-odd"))
    with make_tree(ctx, case.tree) as tree:
        assert_same(device_form(ctx, tree, case), case.want, case.name)


def test_outputs_passed_as_null_stay_untouched(few_workgroups):
    case = C.case(C.names().index("arm-64-odd"))
    optional = [name for name, _ in OUTPUTS if name != "cost"]
    with make_tree(few_workgroups, case.tree) as tree:
        none = device_form(few_workgroups, tree, case, without=optional)
        some = device_form(few_workgroups, tree, case, without=("num_active", "fk_status"))
    assert same_bits(none.cost, case.want.cost)
    for name in optional:
        assert (getattr(none, name) == 77).all(), name
    for name in FIELDS:
        if name in ("num_active", "fk_status"):
            assert (getattr(some, name) == 77).all(), name
        else:
            assert same_bits(getattr(some, name), getattr(case.want, name)), name


@pytest.mark.parametrize("name", ["arm-70", "arm-64-odd", "arm-65-odd-frame"])
def test_equals_the_calls_that_exist_without_it(ctx, name):
    """Context.check_spheres_from_joints for every sphere's clearance and gradient, the hinge in numpy, the summed form of
    Context.clearance_joint_gradient on the poses of Context.forward_kinematics: bit for bit."""
    case = C.case(C.names().index(name))
    with make_tree(ctx, case.tree) as tree:
        flat = ctx.check_spheres_from_joints(case.sdf, C.RESOLUTION, case.xyzr, case.link, tree, case.joint_values,
                                             per_sphere=True, grid_from_world=case.grid_from_world,
                                             rotation=case.rotation, world_from_base=case.world_from_base,
                                             joint_limits=case.joint_limits)
        poses, fk_status = ctx.forward_kinematics(tree, case.joint_values, world_from_base=case.world_from_base,
                                                  joint_limits=case.joint_limits)
        num = len(case.joint_values)
        clearance = np.asarray(flat.sphere_clearance).reshape(num, -1)
        gradient = np.asarray(flat.sphere_gradient).reshape(num, -1, 3)
        c, w = R.hinge(clearance, case.margin)
        value = ~np.isnan(clearance)
        active = value & (w != 0.0)
        without_gradient = active & np.isnan(gradient).any(axis=2)
        summed = ctx.clearance_joint_gradient(tree, poses, case.xyzr, case.link,
                                              sphere_weight=np.where(without_gradient, 0.0, w), sphere_gradient=gradient)
        got = host_form(ctx, tree, case)
    cost = np.empty(num)
    for b in range(num):
        acc = np.float64(0.0)
        for s in np.flatnonzero(value[b]):
            acc = acc + c[b, s]
        cost[b] = acc
    want = capi.ClearanceCosts(cost, np.asarray(summed).reshape(num, -1), active.sum(axis=1).astype(np.int32),
                               (~value).sum(axis=1).astype(np.int32), without_gradient.sum(axis=1).astype(np.int32),
                               np.asarray(fk_status, dtype=np.uint8))
    assert_same(got, want, case.name)
    assert without_gradient.any() == (name != "arm-70")            # (the NaN-gradient rule is part of the odd ones)


def test_device_form_with_links_outside_the_tree_and_without_spheres(few_workgroups):
    """The device form cannot look at the model: a sphere whose link is outside [0, L) is "without a value" (the
    restatement's rule too) and forms no address.  And a model of no spheres: cost +0.0, a gradient row of +0.0, counts 0,
    the kinematics status still there."""
    from oracle import oracle as O
    case = C.case(C.names().index("arm-21"))
    link = np.array(case.link)
    link[[2, 9, 20]] = [case.tree.num_links, -1, 2 ** 31 - 1]
    for model in ((case.xyzr, link), (case.xyzr[:0], link[:0])):
        changed = case._replace(xyzr=np.ascontiguousarray(model[0]), link=np.ascontiguousarray(model[1]))
        if len(model[1]):
            want = R.clearance_cost(O, case.sdf, C.RESOLUTION, changed.xyzr, changed.link, case.tree, case.joint_values,
                                    case.margin, world_from_base=case.world_from_base, joint_limits=case.joint_limits)
            assert (want.num_outside >= 3).all()
        else:
            want = C.case(C.names().index("arm-0")).want._replace(fk_status=case.want.fk_status)
        with make_tree(few_workgroups, case.tree) as tree:
            got = device_form(few_workgroups, tree, changed, num_spheres=len(model[1]))
        print("spheres", len(model[1]), "outside", int(got.num_outside.sum()))
        assert_same(got, want, "%s with %d spheres" % (case.name, len(model[1])))
        if len(model[1]) == 0:
            assert (got.cost.view(np.uint64) == 0).all() and (got.joint_gradient.view(np.uint64) == 0).all()
            assert not got.num_active.any() and not got.num_outside.any() and got.fk_status.any()


def test_trees_at_the_kernels_limits(ctx):
    """A tree of 513 links is rejected; the least chain whose tile is one configuration runs."""
    from oracle import oracle as O
    assert capi.cost_tile_samples(513) == 0
    most = min(n for n in range(1, 513) if capi.cost_tile_samples(n) == 1)
    assert capi.cost_tile_samples(most - 1) == 2
    sdf = body_cases.field(False)
    base = C.motion_cases.world_from_base()
    for links in (513, most):
        t = kinematics_cases.tree("chain-%d" % links)
        xyzr, link = kinematics_cases.sphere_model(t, 5, 31)
        q = (np.random.default_rng(links).random((3, t.num_joints)) * 2.0 - 1.0) * 0.05
        with make_tree(ctx, t) as tree:
            if links == 513:
                with pytest.raises(ValueError, match="512 links, this one has 513"):
                    ctx.clearance_cost(sdf, C.RESOLUTION, xyzr, link, tree, q, C.MARGIN)
                continue
            want = R.clearance_cost(O, sdf, C.RESOLUTION, xyzr, link, t, q, C.MARGIN, world_from_base=base)
            got = ctx.clearance_cost(sdf, C.RESOLUTION, xyzr, link, tree, q, C.MARGIN, world_from_base=base)
        print("chain of", links, "cost", got.cost.tolist(), "active", got.num_active.tolist())
        assert_same(got, want, "chain-%d" % links)


def long_chain(links, spheres):
    """A chain of so many links carrying so many spheres, and B = 3 rows of small joint values (the chain stays in the
    grid) from the first seed for which the restatement has active spheres and a joint gradient that is not zero in at
    least two of the three configurations: a shape whose spheres are all beyond the margin would test nothing.
    -> (tree, xyzr, link, q, want)"""
    from oracle import oracle as O
    sdf = body_cases.field(False)
    base = C.motion_cases.world_from_base()
    t = kinematics_cases.tree("chain-%d" % links)
    xyzr, link = kinematics_cases.sphere_model(t, spheres, 31)
    for seed in range(links, links + 32):
        q = (np.random.default_rng(seed).random((3, t.num_joints)) * 2.0 - 1.0) * 0.05
        want = R.clearance_cost(O, sdf, C.RESOLUTION, xyzr, link, t, q, C.MARGIN, world_from_base=base)
        if ((want.num_active > 0) & (want.joint_gradient != 0.0).any(axis=1)).sum() >= 2:
            return t, xyzr, link, q, want
    raise AssertionError("no seed with active spheres for a chain of %d links" % links)


def assert_long_chain(ctx, links, spheres):
    """Both forms of the kernel on long_chain(links, spheres) against the restatement."""
    sdf = body_cases.field(False)
    base = C.motion_cases.world_from_base()
    t, xyzr, link, q, want = long_chain(links, spheres)
    with make_tree(ctx, t) as tree:
        got = ctx.clearance_cost(sdf, C.RESOLUTION, xyzr, link, tree, q, C.MARGIN, world_from_base=base)
        scored = ctx.clearance_cost(sdf, C.RESOLUTION, xyzr, link, tree, q, C.MARGIN, world_from_base=base,
                                    with_gradient=False)
    print("chain of", links, "with", spheres, "spheres:", capi.cost_launch_geometry(links, spheres, True),
          capi.cost_launch_geometry(links, spheres, False), "active", got.num_active.tolist(), "cost", got.cost.tolist())
    assert_same(got, want, "chain-%d" % links)
    assert scored.joint_gradient is None and scored.num_without_gradient is None
    assert_same(scored, want, "chain-%d, cost only" % links, ("cost", "num_active", "num_outside", "fk_status"))


def test_the_links_on_both_sides_of_the_lds(ctx):
    """What the walk reads of the links, behind the poses of a long chain: the greatest L the launcher still puts into LDS
    in the gradient form at S = 5, by its own geometry, one link more -- which the walk reads through the cache -- and
    the longest chain the kernel takes."""
    spheres = 5
    in_lds = [n for n in range(1, 513) if capi.cost_launch_geometry(n, spheres, True).links_in_lds]
    most = max(in_lds)
    assert in_lds == list(range(1, most + 1)) and most < 512
    assert not capi.cost_launch_geometry(most, spheres, False).links_in_lds          # (the cost-only form has no walk)
    for links in (most, most + 1, 512):
        assert_long_chain(ctx, links, spheres)


def test_fewer_buffered_passes_than_the_tile_has_room_for(ctx):
    """Shapes whose launch buffers fewer passes than the build's limit although the tile has configurations for more,
    because the buffer would not fit next to the poses: S >= 64, so that a pass is one configuration, and every L.  They
    are found with the launcher's own geometry; the longest such chain runs against the restatement.  With the shipped
    constants (tiles of more than one configuration have at most 6 KiB of poses, and four passes take 17 KiB) there is
    none, and the loop of the launcher that halves the passes never turns: this test then only says so."""
    spheres = 70
    limit = max(capi.cost_launch_geometry(n, spheres, True).passes for n in range(1, 513))
    found = [n for n in range(1, 513) for g in [capi.cost_launch_geometry(n, spheres, True)]
             if g.passes < limit and g.passes < g.tile_samples]
    print("buffered passes at the most:", limit, "; chains whose launch has fewer than its tile has room for:", found)
    if found:
        assert_long_chain(ctx, max(found), spheres)


def test_the_two_frame_arguments_are_not_interchangeable(ctx):
    """grid_from_world of the frame and no rotation, against the restatement called the same way, bit for bit: the
    gradients stay in the grid's frame, so the joint gradient is another one than the frame case's."""
    from oracle import oracle as O
    case = C.case(C.names().index("arm-21-frame"))
    want = R.clearance_cost(O, case.sdf, C.RESOLUTION, case.xyzr, case.link, case.tree, case.joint_values, case.margin,
                            case.grid_from_world, None, case.world_from_base, case.joint_limits)
    with make_tree(ctx, case.tree) as tree:
        got = host_form(ctx, tree, case._replace(rotation=None))
    assert_same(got, want, case.name + " without the rotation")
    assert_same(got, case.want, case.name, ("cost", "num_active", "num_outside", "num_without_gradient", "fk_status"))
    finite = np.isfinite(want.joint_gradient) & np.isfinite(case.want.joint_gradient)
    assert np.abs(want.joint_gradient[finite] - case.want.joint_gradient[finite]).max() > 1e-3


def test_argument_errors_that_need_a_tree(ctx):
    """What tests/test_cost_api.py cannot reach without a tree of this context, through the C ABI itself, both forms: NULL
    joint values with B > 0 and J > 0, B * J and B * L of 2^31 or more, and -- the host form, which can look -- a
    sphere's link outside [0, L), the message naming the first offender.  Each is VGT_HIP_ERR_INVALID_ARGUMENT with its
    message, before any device work: the arrays behind the pointers are small host arrays that no rejected call may
    touch, and the outputs stay as they were."""
    lib = ctx._lib
    t = kinematics_cases.tree("arm")                       # L = 8, J = 7
    sdf = body_cases.field(False)
    xyzr, link = kinematics_cases.sphere_model(t, 5, 31)
    xyzr, link = np.ascontiguousarray(xyzr), np.ascontiguousarray(link)
    q = np.zeros((3, t.num_joints))
    outputs = [np.full(3, 9.0), np.full((3, 7), 9.0), np.full(3, 9, np.int32), np.full(3, 9, np.int32),
               np.full(3, 9, np.int32), np.full(3, 9, np.uint8)]
    with make_tree(ctx, t) as tree:
        handle = tree._handle_or_raise()
        for host, fn in ((True, lib.vgt_hip_clearance_cost), (False, lib.vgt_hip_clearance_cost_dev)):
            def refused(needle, link=link, q=capi._ptr(q), num=3, spheres=len(xyzr)):
                rc = fn(ctx.handle, capi._ptr(sdf), *sdf.shape, C.RESOLUTION, None, None, capi._ptr(xyzr), capi._ptr(link),
                        spheres, handle, q, num, None, None, C.MARGIN, 0, *[capi._ptr(o) for o in outputs])
                message = lib.vgt_hip_last_error()
                assert rc == 1 and needle in message, (host, rc, message)

            refused(b"null", q=None)
            # (one sphere, so that B * S stays below 2^31 and the tree's own products are what is refused)
            refused(b"2^31 (configuration, link) pairs", num=2 ** 28, spheres=1)          # 2^28 * 8 = 2^31
            refused(b"2^31 (configuration, joint) pairs", num=(2 ** 31 + 6) // 7, spheres=1)  # the least such B
            if host:
                for first, second in ((t.num_links, -1), (-1, t.num_links), (2 ** 31 - 1, -1)):
                    bad = link.copy()
                    bad[1], bad[3] = first, second
                    refused(b"sphere 1: link %d is not in [0, num_links)" % first, link=bad)
        for o in outputs:
            assert (o == 9).all()
