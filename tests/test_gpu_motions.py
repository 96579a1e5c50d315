"""(gpu) vgt_hip_check_motions[_dev] against tests/motion_ref.py, the CPU restatement: every output bit-equal (NaNs by
position) on the shared cases of tests/motion_cases.py, with and without VGT_HIP_MOTION_STOP_AT_COLLISION -- through the
host form of the product library, and the device form on torch buffers through the testing library limited to two
workgroups, so that 67 motions make the persistent waves stride.  Then the code that exists without this call
(check_spheres_from_joints on the samples, reduced by the restatement's reduction), the optional outputs, an invalid
step count in the device form, trees at the kernel's limits, the argument errors that need a tree, and in the device
form links outside the tree and a model without spheres.

The cases of motion_cases.FRAMED pass a grid_from_world and a rotation (a turn about a general axis), in both forms; one
test passes the first without the second.  The sphere table is run on both sides of the kernel's LDS, the shapes chosen
by the launcher's own geometry (capi.motion_launch_geometry)."""
import numpy as np
import pytest

import body_cases
import kinematics_cases
import motion_cases as C
import motion_ref as R
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu

FIELDS = capi.MotionChecks._fields


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def few_workgroups():
    """A context of the testing library whose motion launches have at most two workgroups."""
    c = capi.Context(0, testing=True)
    c.set_motion_workgroups(2)
    yield c
    c.set_motion_workgroups(0)
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


def assert_same(got, want, what):
    for name in FIELDS:
        g, w = getattr(got, name), getattr(want, name)
        if not same_bits(g, w):
            rows = np.flatnonzero([not same_bits(g[e], w[e]) for e in range(len(w))])
            raise AssertionError("%s: %s differs in motions %s: got %s, want %s"
                                 % (what, name, rows[:8].tolist(), g[rows[:3]].tolist(), w[rows[:3]].tolist()))


def host_form(context, tree, case, stop):
    return context.check_motions(case.sdf, C.RESOLUTION, case.xyzr, case.link, tree, case.joint_from, case.joint_to,
                                 case.num_steps, case.minimum_clearance, case.outside_is_collision, stop,
                                 grid_from_world=case.grid_from_world, rotation=case.rotation,
                                 world_from_base=case.world_from_base, joint_limits=case.joint_limits)


GUARD = 16
OUTPUTS = (("status", 1, "uint8"), ("first_collision", 1, "int32"), ("min_clearance", 1, "float64"),
           ("min_sample", 1, "int32"), ("min_sphere", 1, "int32"), ("min_gradient", 3, "float64"),
           ("fk_status", 1, "uint8"))


def device_form(context, tree, case, stop, without=(), num_steps=None, num_spheres=None):
    """The device form on torch buffers filled with 77, GUARD elements behind each output -> MotionChecks; the outputs
    named in `without` are passed as NULL and come back as they were.  Asserts that the guards are untouched."""
    import torch
    motions = len(case.joint_from)
    steps = case.num_steps if num_steps is None else num_steps
    inputs = [case.sdf, case.xyzr, case.link, case.joint_from, case.joint_to]
    if case.tree.num_joints == 0:
        inputs[3] = inputs[4] = np.zeros(1)
    dev = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in inputs]
    steps_dev = None if np.ndim(steps) == 0 else torch.from_numpy(np.ascontiguousarray(steps, dtype=np.int32)).cuda()
    out = {name: torch.full((motions * width + GUARD,), 77, dtype=getattr(torch, dtype), device="cuda")
           for name, width, dtype in OUTPUTS}
    torch.cuda.synchronize()
    pointers = {name + "_ptr": None if name in without else out[name].data_ptr() for name in out if name != "status"}
    context.check_motions_dev(dev[0].data_ptr(), case.sdf.shape, C.RESOLUTION, dev[1].data_ptr(), dev[2].data_ptr(),
                              len(case.xyzr) if num_spheres is None else num_spheres, tree, dev[3].data_ptr(),
                              dev[4].data_ptr(),
                              int(steps) if steps_dev is None else 0, motions, out["status"].data_ptr(),
                              minimum_clearance=case.minimum_clearance, outside_is_collision=case.outside_is_collision,
                              stop_at_collision=stop, grid_from_world=case.grid_from_world, rotation=case.rotation,
                              world_from_base=case.world_from_base,
                              joint_limits=case.joint_limits,
                              num_steps_ptr=None if steps_dev is None else steps_dev.data_ptr(), **pointers)
    context.synchronize()
    got = []
    for name, width, _ in OUTPUTS:
        flat = out[name].cpu().numpy()
        assert (flat[motions * width:] == 77).all(), "the guard behind %s" % name
        flat = flat[:motions * width]
        got.append(flat.reshape(motions, 3) if width == 3 else flat)
    return capi.MotionChecks(*got)


def report(case, got):
    print(case.name, "statuses", np.bincount(got.status, minlength=4).tolist(), "tile",
          capi.motion_tile_samples(case.tree.num_links))


@pytest.mark.parametrize("stop", [False, True], ids=["all", "stop"])
@pytest.mark.parametrize("index", range(len(C.CASES)), ids=C.names())
def test_host_form(ctx, index, stop):
    case = C.case(index)
    with make_tree(ctx, case.tree) as tree:
        got = host_form(ctx, tree, case, stop)
    report(case, got)
    assert_same(got, case.want_stopped if stop else case.want, case.name)


@pytest.mark.parametrize("stop", [False, True], ids=["all", "stop"])
@pytest.mark.parametrize("index", range(len(C.CASES)), ids=C.names())
def test_device_form_with_striding_waves(few_workgroups, index, stop):
    case = C.case(index)
    with make_tree(few_workgroups, case.tree) as tree:
        got = device_form(few_workgroups, tree, case, stop)
    report(case, got)
    assert_same(got, case.want_stopped if stop else case.want, case.name)


def test_device_form_of_the_product_library(ctx):
    case = C.case(3)
    with make_tree(ctx, case.tree) as tree:
        assert_same(device_form(ctx, tree, case, False), case.want, case.name)
        assert_same(device_form(ctx, tree, case, True), case.want_stopped, case.name)


def test_outputs_passed_as_null_stay_untouched(few_workgroups):
    case = C.case(1)
    optional = [name for name, _, _ in OUTPUTS if name != "status"]
    with make_tree(few_workgroups, case.tree) as tree:
        none = device_form(few_workgroups, tree, case, False, without=optional)
        some = device_form(few_workgroups, tree, case, True, without=("min_clearance", "min_gradient", "fk_status"))
    assert same_bits(none.status, case.want.status)
    for name in optional:
        assert (getattr(none, name) == 77).all(), name
    for name in FIELDS:
        if name in ("min_clearance", "min_gradient", "fk_status"):
            assert (getattr(some, name) == 77).all(), name
        else:
            assert same_bits(getattr(some, name), getattr(case.want_stopped, name)), name


FIRST_FRAMED = min(C.FRAMED)


@pytest.mark.parametrize("index", [0, 3, FIRST_FRAMED], ids=[C.names()[0], C.names()[3], C.names()[FIRST_FRAMED]])
def test_equals_the_calls_that_exist_without_it(ctx, index):
    """The samples interpolated in numpy, Context.check_spheres_from_joints on them, the restatement's reduction."""
    case = C.case(index)
    q, first = R.interpolate(case.joint_from, case.joint_to, case.num_steps)
    with make_tree(ctx, case.tree) as tree:
        flat = ctx.check_spheres_from_joints(case.sdf, C.RESOLUTION, case.xyzr, case.link, tree, q,
                                             minimum_clearance=case.minimum_clearance,
                                             outside_is_collision=case.outside_is_collision,
                                             grid_from_world=case.grid_from_world, rotation=case.rotation,
                                             world_from_base=case.world_from_base, joint_limits=case.joint_limits)
        samples = R.Samples(flat.status, flat.min_clearance, flat.min_sphere, flat.min_gradient, flat.fk_status)
        for stop in (False, True):
            assert_same(host_form(ctx, tree, case, stop), R.reduce_motions(samples, first, stop), case.name)


def test_a_negative_step_count_in_the_device_form(few_workgroups):
    case = C.case(0)
    steps = np.array(case.num_steps, dtype=np.int32)
    steps[[0, 11, 66]] = [-1, -7, -2147483648]
    with make_tree(few_workgroups, case.tree) as tree:
        got = device_form(few_workgroups, tree, case, False, num_steps=steps)
    invalid = steps < 0
    assert (got.status[invalid] == capi.MOTION_INVALID).all() and (got.first_collision[invalid] == -1).all()
    assert np.isnan(got.min_clearance[invalid]).all() and np.isnan(got.min_gradient[invalid]).all()
    assert (got.min_sample[invalid] == -1).all() and (got.min_sphere[invalid] == -1).all()
    assert (got.fk_status[invalid] == 0).all()
    for name in FIELDS:
        assert same_bits(getattr(got, name)[~invalid], getattr(case.want, name)[~invalid]), name


def test_trees_at_the_kernels_limits(ctx):
    """A tree of 641 links is rejected; the least chain whose tile is one sample runs."""
    assert capi.motion_tile_samples(641) == 0
    most = min(n for n in range(1, 641) if capi.motion_tile_samples(n) == 1)
    assert capi.motion_tile_samples(most - 1) == 2
    sdf = body_cases.field(False)
    for links in (641, most):
        t = kinematics_cases.tree("chain-%d" % links)
        xyzr, link = kinematics_cases.sphere_model(t, 5, 31)
        rng = np.random.default_rng(links)
        joint_from = (rng.random((3, t.num_joints)) * 2.0 - 1.0) * 0.05
        joint_to = joint_from + (rng.random((3, t.num_joints)) * 2.0 - 1.0) * 0.05
        with make_tree(ctx, t) as tree:
            if links == 641:
                with pytest.raises(ValueError, match="640 links, this one has 641"):
                    ctx.check_motions(sdf, C.RESOLUTION, xyzr, link, tree, joint_from, joint_to, 2)
                continue
            from oracle import oracle as O
            want = R.check_motions(O, sdf, C.RESOLUTION, xyzr, link, t, joint_from, joint_to, 2,
                                   world_from_base=C.world_from_base())
            got = ctx.check_motions(sdf, C.RESOLUTION, xyzr, link, tree, joint_from, joint_to, 2,
                                    world_from_base=C.world_from_base())
        print("chain of", links, "statuses", got.status.tolist(), "min_sample", got.min_sample.tolist())
        assert_same(got, want, "chain-%d" % links)


def test_the_sphere_table_on_both_sides_of_the_lds(ctx):
    """The table of the model behind 60 KiB of poses: at 640 links the greatest S the launcher still puts into LDS, by its
    own geometry, and one sphere more, which the kernel reads through the cache; and the models of the shared cases on
    both sides of the table's own limit.  A chain of 640 links, 5 motions of 0, 1, 2, 3 and 5 steps with joint values of
    a few thousandths, so that the chain stays in the grid; the threshold lies between the motions' least clearances."""
    from oracle import oracle as O
    names = C.names()
    for name, in_lds in (("arm-70", 1), ("arm-257", 0), ("arm-257-odd-frame", 0)):
        case = C.case(names.index(name))
        assert capi.motion_launch_geometry(case.tree.num_links, len(case.xyzr)).table_in_lds == in_lds, name
    links = 640
    assert capi.motion_launch_geometry(links, 1).table_in_lds == 1
    most = max(s for s in range(1, 1024) if capi.motion_launch_geometry(links, s).table_in_lds)
    assert capi.motion_launch_geometry(links, most + 1).table_in_lds == 0
    sdf = body_cases.field(False)
    t = kinematics_cases.tree("chain-%d" % links)
    steps = np.array([0, 1, 2, 3, 5], dtype=np.int32)
    rng = np.random.default_rng(links)
    joint_from = (rng.random((5, t.num_joints)) * 2.0 - 1.0) * 0.004
    joint_to = joint_from + (rng.random((5, t.num_joints)) * 2.0 - 1.0) * 0.004
    base = C.world_from_base()
    with make_tree(ctx, t) as tree:
        for spheres in (most, most + 1):
            xyzr, link = kinematics_cases.sphere_model(t, spheres, 31)
            least = R.check_motions(O, sdf, C.RESOLUTION, xyzr, link, t, joint_from, joint_to, steps,
                                    world_from_base=base).min_clearance
            least = np.unique(least[np.isfinite(least)])
            assert len(least) >= 2
            threshold = float((least[(len(least) - 1) // 2] + least[(len(least) - 1) // 2 + 1]) * 0.5)
            second_slice = False
            for stop in (False, True):
                want = R.check_motions(O, sdf, C.RESOLUTION, xyzr, link, t, joint_from, joint_to, steps, threshold,
                                       stop_at_collision=stop, world_from_base=base)
                got = ctx.check_motions(sdf, C.RESOLUTION, xyzr, link, tree, joint_from, joint_to, steps, threshold,
                                        stop_at_collision=stop, world_from_base=base)
                print("chain of", links, "with", spheres, "spheres, stop", stop, "statuses", got.status.tolist(),
                      "min_sample", got.min_sample.tolist(), "min_sphere", got.min_sphere.tolist())
                assert_same(got, want, "chain-%d with %d spheres" % (links, spheres))
                assert len(set(want.status.tolist())) > 1
                second_slice = second_slice or bool((want.min_sphere >= 64).any())
            assert second_slice or spheres == most


def test_the_two_frame_arguments_are_not_interchangeable(ctx):
    """grid_from_world of the frame and no rotation: the same cells, so clearances, statuses and indices are the frame
    case's bit for bit, and min_gradient stays in the grid's frame -- the frame case's turned back (g * rotation for a row
    vector g), within 1e-12: another order of operations, so not bit for bit.  An entry point that drops one of the two
    pointers, or swaps them, fails here or in the frame cases."""
    case = C.case(FIRST_FRAMED)
    r = case.rotation.reshape(3, 3)
    with make_tree(ctx, case.tree) as tree:
        for stop in (False, True):
            want = case.want_stopped if stop else case.want
            got = host_form(ctx, tree, case._replace(rotation=None), stop)
            for name in FIELDS:
                if name != "min_gradient":
                    assert same_bits(getattr(got, name), getattr(want, name)), name
            g = want.min_gradient
            back = np.stack([(g[:, 0] * r[0, i] + g[:, 1] * r[1, i]) + g[:, 2] * r[2, i] for i in range(3)], axis=-1)
            finite = np.isfinite(back)
            assert finite.any() and np.array_equal(np.isfinite(got.min_gradient), finite)
            worst = float(np.abs(got.min_gradient[finite] - back[finite]).max())
            moved = float(np.abs(got.min_gradient[finite] - g[finite]).max())
            print("stop", stop, "largest difference", worst, "and from the turned gradients", moved)
            assert worst <= 1e-12 and moved > 1e-3


def test_argument_errors_that_need_a_tree(ctx):
    """What tests/test_motion_api.py cannot reach without a tree of this context, through the C ABI itself, both forms:
    NULL joint arrays with E > 0 and J > 0, E * J of 2^31 or more, and -- the host form, which can look -- a sphere's
    link outside [0, L), the message naming the first offender.  Each is VGT_HIP_ERR_INVALID_ARGUMENT with its message,
    before any device work: the arrays behind the pointers are small host arrays that no rejected call may touch, and
    the outputs stay as they were."""
    lib = ctx._lib
    t = kinematics_cases.tree("arm")                       # L = 8, J = 7
    sdf = body_cases.field(False)
    xyzr, link = kinematics_cases.sphere_model(t, 5, 31)
    xyzr, link = np.ascontiguousarray(xyzr), np.ascontiguousarray(link)
    a, b = np.zeros((3, t.num_joints)), np.ones((3, t.num_joints))
    outputs = [np.full(3, 9, np.uint8), np.full(3, 9, np.int32), np.full(3, 9.0), np.full(3, 9, np.int32),
               np.full(3, 9, np.int32), np.full((3, 3), 9.0), np.full(3, 9, np.uint8)]
    with make_tree(ctx, t) as tree:
        handle = tree._handle_or_raise()
        for host, fn in ((True, lib.vgt_hip_check_motions), (False, lib.vgt_hip_check_motions_dev)):
            def refused(needle, link=link, a=capi._ptr(a), b=capi._ptr(b), motions=3):
                rc = fn(ctx.handle, capi._ptr(sdf), *sdf.shape, C.RESOLUTION, None, None, capi._ptr(xyzr), capi._ptr(link),
                        len(xyzr), handle, a, b, None, 2, motions, None, None, 0.0, 0, *[capi._ptr(o) for o in outputs])
                message = lib.vgt_hip_last_error()
                assert rc == 1 and needle in message, (host, rc, message)

            refused(b"null", a=None)
            refused(b"null", b=None)
            refused(b"null", a=None, b=None)
            refused(b"2^31 (motion, joint) pairs", motions=2 ** 30)            # 2^30 * 7 >= 2^31
            refused(b"2^31 (motion, joint) pairs", motions=(2 ** 31 + 6) // 7)  # the least such E
            if host:
                for first, second in ((t.num_links, -1), (-1, t.num_links), (2 ** 31 - 1, -1)):
                    bad = link.copy()
                    bad[1], bad[3] = first, second
                    refused(b"sphere 1: link %d is not in [0, num_links)" % first, link=bad)
        for o in outputs:
            assert (o == 9).all()


@pytest.mark.parametrize("stop", [False, True], ids=["all", "stop"])
def test_device_form_with_links_outside_the_tree_and_without_spheres(few_workgroups, stop):
    """The device form cannot look at the model: a sphere whose link is outside [0, L) is "without a value", as in
    vgt_hip_check_spheres_dev (the restatement's rule too).  And a model of no spheres: every sample is NO_VALUE, the
    kinematics status is still there."""
    from oracle import oracle as O
    case = C.case(0)                                       # arm-21: a sphere outside the grid is no collision
    link = np.array(case.link)
    link[[2, 9, 20]] = [case.tree.num_links, -1, 2 ** 31 - 1]
    for model in ((case.xyzr, link), (case.xyzr[:0], link[:0])):
        changed = case._replace(xyzr=np.ascontiguousarray(model[0]), link=np.ascontiguousarray(model[1]))
        want = R.check_motions(O, case.sdf, C.RESOLUTION, changed.xyzr, changed.link, case.tree, case.joint_from,
                               case.joint_to, case.num_steps, case.minimum_clearance, case.outside_is_collision, stop,
                               world_from_base=case.world_from_base, joint_limits=case.joint_limits)
        if len(changed.link) == 0:                         # (torch has no pointer for an empty tensor: one element stands in)
            changed = changed._replace(xyzr=np.zeros((1, 4)), link=np.zeros(1, np.int32))
        with make_tree(few_workgroups, case.tree) as tree:
            got = device_form(few_workgroups, tree, changed, stop, num_spheres=len(model[1]))
        print("spheres", len(model[1]), "statuses", np.bincount(got.status, minlength=4).tolist())
        assert_same(got, want, "%s with %d spheres" % (case.name, len(model[1])))
        if len(model[1]) == 0:
            assert (got.status == capi.MOTION_NO_VALUE).all() and (got.min_sample == -1).all() and got.fk_status.any()
