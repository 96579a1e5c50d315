"""(gpu) vgt_hip_check_self_collision[_poses][_dev] against tests/self_ref.py, the CPU restatement: every output bit-equal
(NaNs by position) on the shared cases of tests/self_cases.py -- through the host form of the product library, and the
device form on torch buffers through the testing library limited to one and to three workgroups, so that the persistent
waves stride, and with the default.  Then pair lists of every length around the lanes of a configuration, the poses form
on the poses vgt_hip_forward_kinematics_dev wrote, the summed vgt_hip_clearance_joint_gradient_dev on the call's own
min_pair and min_direction, in the device form sphere indices and links out of range, outputs passed as NULL, models at
the kernel's limits, and the argument errors that need a tree or a context."""
import functools

import numpy as np
import pytest

import kinematics_cases
import self_cases as C
import self_ref as R
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu

FIELDS = capi.SelfCollisionChecks._fields
GUARD = 16
OUTPUTS = (("status", "uint8"), ("num_below", "int32"), ("num_without_value", "int32"), ("min_clearance", "float64"),
           ("min_pair", "int32"), ("min_direction", "float64"), ("joint_gradient", "float64"), ("fk_status", "uint8"),
           ("pair_clearance", "float64"))


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def testing_ctx():
    c = capi.Context(0, testing=True)
    yield c
    c.set_self_collision_workgroups(0)
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
        if w is None or g is None:                         # (what one of the two forms does not have)
            continue
        if not same_bits(g, w):
            rows = np.flatnonzero([not same_bits(g[e], w[e]) for e in range(len(w))])
            raise AssertionError("%s: %s differs in configurations %s: got %s, want %s"
                                 % (what, name, rows[:8].tolist(), g[rows[:3]].tolist(), w[rows[:3]].tolist()))


def host_form(context, tree, case, **kw):
    return context.check_self_collision(case.xyzr, case.link, case.pairs, tree, case.joint_values,
                                        case.minimum_clearance, case.no_value_is_collision, per_pair=True,
                                        world_from_base=case.world_from_base, joint_limits=case.joint_limits, **kw)


def _on_device(array, stand_in):
    import torch
    array = np.asarray(array)
    return torch.from_numpy(np.array(array if array.size else stand_in)).cuda()     # (copies: the cases are read-only)


def device_form(context, tree, case, without=(), poses=False, num_spheres=None, num_pairs=None):
    """The device form on torch buffers filled with 77, GUARD elements behind each output -> SelfCollisionChecks; the
    outputs named in `without` are passed as NULL and come back as they were.  poses: the poses form, on the poses
    forward_kinematics_dev writes first.  Asserts that the guards are untouched."""
    import torch
    num, joints = case.joint_values.shape
    count, pairs = len(case.link), len(case.pairs)
    spheres = count if num_spheres is None else num_spheres
    listed = pairs if num_pairs is None else num_pairs
    xyzr = _on_device(case.xyzr, np.zeros((1, 4)))         # (torch has no pointer for an empty tensor: one element stands in)
    link = _on_device(case.link, np.zeros(1, np.int32))
    ab = _on_device(case.pairs, np.zeros((1, 2), np.int32))
    q = _on_device(case.joint_values, np.zeros(1))
    widths = {"min_direction": 3, "joint_gradient": joints, "pair_clearance": listed}
    out = {name: torch.full((num * widths.get(name, 1) + GUARD,), 77, dtype=getattr(torch, dtype), device="cuda")
           for name, dtype in OUTPUTS}
    torch.cuda.synchronize()
    pointers = {name + "_ptr": None if name in without else out[name].data_ptr() for name in out
                if name != "status" and not (poses and name == "fk_status")}
    if poses:
        links = case.tree.num_links
        link_poses = torch.full((num * links * 16,), 5.0, dtype=torch.float64, device="cuda")
        context.forward_kinematics_dev(tree, q.data_ptr(), num, link_poses.data_ptr(), world_from_base=case.world_from_base,
                                       joint_limits=case.joint_limits)
        context.check_self_collision_poses_dev(
            xyzr.data_ptr(), link.data_ptr(), spheres, ab.data_ptr(), listed, link_poses.data_ptr(), num, links,
            out["status"].data_ptr(), tree=None if "joint_gradient" in without else tree,
            minimum_clearance=case.minimum_clearance, flags=int(case.no_value_is_collision), **pointers)
    else:
        context.check_self_collision_dev(
            xyzr.data_ptr(), link.data_ptr(), spheres, ab.data_ptr(), listed, tree, q.data_ptr(), num,
            out["status"].data_ptr(), minimum_clearance=case.minimum_clearance, world_from_base=case.world_from_base,
            joint_limits=case.joint_limits, flags=int(case.no_value_is_collision), **pointers)
    context.synchronize()
    got = []
    for name, _ in OUTPUTS:
        width = widths.get(name, 1)
        flat = out[name].cpu().numpy()
        assert (flat[num * width:] == 77).all(), "the guard behind %s" % name
        flat = flat[:num * width]
        got.append(flat.reshape(num, width) if name in widths else flat)
    if poses:
        got[7] = None
    return capi.SelfCollisionChecks(*got)


def untouched(checks, names):
    return all((getattr(checks, name) == 77).all() for name in names)


def report(case, got):
    print(case.name, "P", len(case.pairs), "below", int(got.num_below.sum()), "without a value",
          int(got.num_without_value.sum()), "statuses", np.bincount(got.status, minlength=3).tolist(), "tile",
          capi.self_collision_tile_samples(case.tree.num_links, len(case.link)))


def test_tile_query_is_what_the_header_says():
    for links, spheres in [(1, 0), (1, 21), (8, 16), (8, 21), (8, 64), (8, 200), (15, 200), (8, 257), (18, 21), (80, 21),
                           (81, 21), (680, 0), (681, 0), (1, 2037), (1, 2038), (0, 5), (-1, 5), (5, -1), (2 ** 40, 1),
                           (1, 2 ** 40)]:
        want = C.tile_formula(links, spheres) if links > 0 and spheres >= 0 else 0
        assert capi.self_collision_tile_samples(links, spheres) == want, (links, spheres)
    assert capi.self_collision_tile_samples(8, 21) == 8          # (what the batch sizes and pair counts below sit around)


@pytest.mark.parametrize("index", range(len(C.CASES)), ids=C.names())
def test_host_form(ctx, index):
    case = C.case(index)
    with make_tree(ctx, case.tree) as tree:
        got = host_form(ctx, tree, case)
    report(case, got)
    assert_same(got, case.want, case.name)


@pytest.mark.parametrize("workgroups", [1, 3, 0])
@pytest.mark.parametrize("index", range(len(C.CASES)), ids=C.names())
def test_device_form_with_striding_waves(testing_ctx, index, workgroups):
    case = C.case(index)
    testing_ctx.set_self_collision_workgroups(workgroups)
    with make_tree(testing_ctx, case.tree) as tree:
        got = device_form(testing_ctx, tree, case)
    assert_same(got, case.want, case.name)
    if len(case.link) == 0:
        assert untouched(got, ["pair_clearance"])


def test_device_form_of_the_product_library(ctx):
    case = C.case(C.names().index("body-21"))
    with make_tree(ctx, case.tree) as tree:
        assert_same(device_form(ctx, tree, case), case.want, case.name)


POSES = ["fixed1-21", "arm-21", "arm-257", "body-65-m0", C.names()[8], C.names()[9], "arm-0-m0", "arm-21-B9"]


@pytest.mark.parametrize("name", POSES)
def test_poses_form_on_the_poses_of_the_forward_kinematics(testing_ctx, name):
    """The same kernel with another phase A: bit-equal to the joint-value form and to the restatement, fk_status aside;
    without a tree there is no gradient, and the rest is the same."""
    case = C.case(C.names().index(name))
    testing_ctx.set_self_collision_workgroups(2)
    with make_tree(testing_ctx, case.tree) as tree:
        from_joints = device_form(testing_ctx, tree, case)
        from_poses = device_form(testing_ctx, tree, case, poses=True)
        without_tree = device_form(testing_ctx, tree, case, poses=True, without=("joint_gradient",))
    assert from_poses.fk_status is None
    assert_same(from_poses, from_joints, case.name)
    assert_same(from_poses, case.want, case.name)
    assert untouched(without_tree, ["joint_gradient"])
    assert_same(without_tree, case.want, case.name, [f for f in FIELDS if f != "joint_gradient"])


def test_host_poses_form(ctx):
    case = C.case(C.names().index("body-21"))
    with make_tree(ctx, case.tree) as tree:
        got = ctx.check_self_collision_poses(case.xyzr, case.link, case.pairs, case.poses, tree, case.minimum_clearance,
                                             case.no_value_is_collision, per_pair=True)
        bare = ctx.check_self_collision_poses(case.xyzr, case.link, case.pairs, case.poses, None, case.minimum_clearance,
                                              case.no_value_is_collision)
    assert got.fk_status is None and bare.joint_gradient is None and bare.pair_clearance is None
    assert_same(got, case.want, case.name)
    assert_same(bare, case.want, case.name)


@functools.lru_cache(maxsize=None)
def _shortened(num_pairs):
    """arm-21 with the first num_pairs entries of a list that starts with its planted pairs."""
    case = C.case(C.names().index("arm-21"))
    pairs = np.concatenate([case.pairs[-6:], case.pairs[:-6]])[:num_pairs]
    want = R.check_self_collision(case.xyzr, case.link, pairs, case.tree, case.joint_values, case.minimum_clearance,
                                  case.no_value_is_collision, case.world_from_base, case.joint_limits)
    return case._replace(pairs=np.ascontiguousarray(pairs), want=want, name="arm-21-P%d" % num_pairs)


def pair_counts():
    per_configuration = 64 // C.tile_formula(8, 21)
    return sorted({0, 1, per_configuration - 1, per_configuration, per_configuration + 1, 63, 64, 65})


@pytest.mark.parametrize("num_pairs", pair_counts())
def test_pair_lists_around_the_lanes_of_a_configuration(ctx, testing_ctx, num_pairs):
    case = _shortened(num_pairs)
    assert len(case.pairs) == num_pairs
    testing_ctx.set_self_collision_workgroups(3)
    with make_tree(testing_ctx, case.tree) as tree:
        got = device_form(testing_ctx, tree, case)
    report(case, got)
    assert_same(got, case.want, case.name)
    with make_tree(ctx, case.tree) as tree:
        assert_same(host_form(ctx, tree, case), case.want, case.name)
    if num_pairs == 0:
        assert (got.status == capi.SELF_NO_VALUE).all() and (got.min_pair == -1).all()
        assert np.isnan(got.min_clearance).all() and np.isnan(got.joint_gradient).all()
        assert not got.num_below.any() and not got.num_without_value.any()


@pytest.mark.parametrize("name", ["arm-65", "body-21"])
def test_equals_the_calls_that_exist_without_it(ctx, name):
    """joint_gradient against the summed form of vgt_hip_clearance_joint_gradient_dev on the poses of
    vgt_hip_forward_kinematics_dev, with the two-entry weights built from the call's own min_pair and min_direction: bit
    for bit (a NaN row where there is no worst pair, which the summed form does not know)."""
    import torch
    case = C.case(C.names().index(name))
    num, joints = case.joint_values.shape
    count, links = len(case.link), case.tree.num_links
    with make_tree(ctx, case.tree) as tree:
        got = device_form(ctx, tree, case)
        weight = np.zeros((num, count))
        gradient = np.zeros((num, count, 3))
        found = np.flatnonzero(got.min_pair >= 0)
        a, b = case.pairs[got.min_pair[found], 0], case.pairs[got.min_pair[found], 1]
        weight[found, a] = weight[found, b] = 1.0
        gradient[found, a] = got.min_direction[found]
        gradient[found, b] = -got.min_direction[found]
        dev = [torch.from_numpy(np.array(x)).cuda() for x in (case.joint_values, case.xyzr, case.link, weight, gradient)]
        poses = torch.zeros(num * links * 16, dtype=torch.float64, device="cuda")
        summed = torch.full((num * joints,), 77.0, dtype=torch.float64, device="cuda")
        ctx.forward_kinematics_dev(tree, dev[0].data_ptr(), num, poses.data_ptr(), world_from_base=case.world_from_base,
                                   joint_limits=case.joint_limits)
        ctx.clearance_joint_gradient_dev(tree, poses.data_ptr(), num, dev[1].data_ptr(), dev[2].data_ptr(), count,
                                         summed.data_ptr(), sphere_weight_ptr=dev[3].data_ptr(),
                                         sphere_gradient_ptr=dev[4].data_ptr())
        ctx.synchronize()
    want = summed.cpu().numpy().reshape(num, joints)
    want[got.min_pair < 0] = np.nan
    assert len(found) > 40 and np.isfinite(want).any() and np.isnan(want[found]).any()
    assert same_bits(got.joint_gradient, want)


def test_device_form_with_spheres_and_links_out_of_range(testing_ctx):
    """The device form cannot look at the model or the list: a pair with a sphere outside [0, S), and a sphere whose link
    is outside [0, L), are "without a value" (the restatement's rule too) and form no address."""
    case = C.case(C.names().index("arm-21"))
    count = len(case.link)
    link = np.array(case.link)
    link[[2, 9]] = [case.tree.num_links, -1]
    link[11] = 2 ** 31 - 1
    pairs = np.array(case.pairs)
    pairs[[1, 7, 20, 33]] = [[-1, 3], [4, count], [2 ** 31 - 1, 5], [-2 ** 31, 2 ** 31 - 1]]
    want = R.check_self_collision(case.xyzr, link, pairs, case.tree, case.joint_values, case.minimum_clearance,
                                  case.no_value_is_collision, case.world_from_base, case.joint_limits)
    assert (want.num_without_value >= 4 + 3).all() and np.isnan(want.pair_clearance[:, [1, 7, 20, 33]]).all()
    changed = case._replace(link=link, pairs=pairs)
    for workgroups in (1, 0):
        testing_ctx.set_self_collision_workgroups(workgroups)
        with make_tree(testing_ctx, case.tree) as tree:
            got = device_form(testing_ctx, tree, changed)
            from_poses = device_form(testing_ctx, tree, changed, poses=True)
        assert_same(got, want, "arm-21 with pairs and links out of range")
        assert_same(from_poses, want, "arm-21 with pairs and links out of range, poses form")
    # fewer spheres than the list knows: the pairs beyond them are without a value
    fewer = R.check_self_collision(case.xyzr[:10], case.link[:10], case.pairs, case.tree, case.joint_values,
                                   case.minimum_clearance, case.no_value_is_collision, case.world_from_base,
                                   case.joint_limits)
    with make_tree(testing_ctx, case.tree) as tree:
        got = device_form(testing_ctx, tree, case, num_spheres=10)
    assert_same(got, fewer, "arm-21 with ten spheres")


def test_outputs_passed_as_null_stay_untouched(testing_ctx):
    case = C.case(C.names().index("body-21"))
    optional = [name for name, _ in OUTPUTS if name != "status"]
    testing_ctx.set_self_collision_workgroups(2)
    with make_tree(testing_ctx, case.tree) as tree:
        none = device_form(testing_ctx, tree, case, without=optional)
        some = device_form(testing_ctx, tree, case, without=("num_below", "min_pair", "min_direction", "fk_status"))
        other = device_form(testing_ctx, tree, case, without=("joint_gradient", "min_clearance", "pair_clearance"))
    assert same_bits(none.status, case.want.status) and untouched(none, optional)
    assert untouched(some, ["num_below", "min_pair", "min_direction", "fk_status"])
    assert_same(some, case.want, case.name, [f for f in FIELDS if f not in ("num_below", "min_pair", "min_direction",
                                                                             "fk_status")])
    assert untouched(other, ["joint_gradient", "min_clearance", "pair_clearance"])
    assert_same(other, case.want, case.name, [f for f in FIELDS if f not in ("joint_gradient", "min_clearance",
                                                                              "pair_clearance")])


def test_models_at_the_kernels_limits(ctx):
    """2037 spheres on one link run, 2038 are refused; a chain of 681 links is refused."""
    t = kinematics_cases.tree("fixed1")
    xyzr, link = kinematics_cases.sphere_model(t, 2038, 5)
    pairs = np.array([[0, 2036], [5, 2035], [2035, 2036], [7, 1000], [1, 2]], np.int32)
    with make_tree(ctx, t) as tree:
        want = R.check_self_collision(xyzr[:2037], link[:2037], pairs, t, np.zeros((3, 0)))
        got = ctx.check_self_collision(xyzr[:2037], link[:2037], pairs, tree, np.zeros((3, 0)), per_pair=True)
        assert_same(got, want, "2037 spheres")
        assert np.isfinite(got.min_clearance).all()
        with pytest.raises(ValueError, match="this model has 1 links and 2038 spheres"):
            ctx.check_self_collision(xyzr, link, pairs, tree, np.zeros((3, 0)))
    t = kinematics_cases.tree("chain-681")
    with make_tree(ctx, t) as tree:
        with pytest.raises(ValueError, match="this model has 681 links and 2 spheres"):
            ctx.check_self_collision(xyzr[:2], [0, 680], [[0, 1]], tree, np.zeros((1, t.num_joints)))


def test_argument_errors_that_need_a_tree_or_a_context(ctx):
    """Through the C ABI itself, every form: each is VGT_HIP_ERR_INVALID_ARGUMENT with its message, before any device
    work: the arrays behind the pointers are small host arrays that no rejected call may touch, and the outputs stay as
    they were."""
    lib = ctx._lib
    t = kinematics_cases.tree("arm")                       # L = 8, J = 7
    xyzr, link = kinematics_cases.sphere_model(t, 5, 31)
    xyzr, link = np.ascontiguousarray(xyzr), np.ascontiguousarray(link)
    pairs = np.array([[0, 1], [1, 4], [2, 3], [0, 4]], np.int32)
    q = np.zeros((3, t.num_joints))
    poses = np.zeros((3, t.num_links, 16))
    outputs = [np.full(3, 9, np.uint8), np.full(3, 9, np.int32), np.full(3, 9, np.int32), np.full(3, 9.0),
               np.full(3, 9, np.int32), np.full((3, 3), 9.0), np.full((3, 7), 9.0), np.full(3, 9, np.uint8),
               np.full((3, 4), 9.0)]
    other = capi.Context(0)
    with make_tree(ctx, t) as tree, make_tree(other, t) as foreign, \
            make_tree(ctx, kinematics_cases.tree("body")) as body:
        handle = tree._handle_or_raise()
        for host in (True, False):
            def joints(needle, xyzr=xyzr, link=link, pairs=pairs, num_pairs=4, spheres=5, tree=handle, q=capi._ptr(q),
                       num=3, minimum=0.0, flags=0, status=True, clearance=True, context=ctx.handle):
                fn = lib.vgt_hip_check_self_collision if host else lib.vgt_hip_check_self_collision_dev
                out = [capi._ptr(o) for o in outputs]
                rc = fn(context, capi._ptr(xyzr), capi._ptr(link), spheres, capi._ptr(pairs), num_pairs, tree, q, num,
                        None, None, minimum, flags, out[0] if status else None, *out[1:8], out[8] if clearance else None)
                message = lib.vgt_hip_last_error()
                assert rc == 1 and needle in message, (host, rc, message)

            def from_poses(needle, link=link, pairs=pairs, tree=handle, links=t.num_links, num=3, gradient=True,
                           link_poses=capi._ptr(poses), flags=0, minimum=0.0):
                fn = lib.vgt_hip_check_self_collision_poses if host else lib.vgt_hip_check_self_collision_poses_dev
                out = [capi._ptr(o) for o in outputs]
                rc = fn(ctx.handle, capi._ptr(xyzr), capi._ptr(link), 5, capi._ptr(pairs), 4, link_poses, num, links,
                        tree, minimum, flags, *out[:6], out[6] if gradient else None, out[8])
                message = lib.vgt_hip_last_error()
                assert rc == 1 and needle in message, (host, rc, message)

            joints(b"null", context=None)
            joints(b"null", status=False)
            joints(b"null", tree=None)
            joints(b"null", xyzr=None)
            joints(b"null", link=None)
            joints(b"null", pairs=None)
            joints(b"null", q=None)
            joints(b"minimum_clearance must not be NaN", minimum=np.nan)
            joints(b"unknown self-collision flag", flags=2)
            joints(b"must not be negative", num=-1)
            joints(b"must not be negative", spheres=-1)
            joints(b"must not be negative", num_pairs=-1)
            joints(b"fewer than 2^31 spheres, pairs and configurations", num=2 ** 31)
            joints(b"fewer than 2^31 spheres, pairs and configurations", num_pairs=2 ** 31, clearance=False)
            joints(b"2^31 (configuration, pair) clearances", num=2 ** 29)                      # 2^29 * 4 = 2^31
            joints(b"2^31 (configuration, link) pairs", num=2 ** 28, clearance=False)           # 2^28 * 8 = 2^31
            joints(b"2^31 (configuration, joint) pairs", num=(2 ** 31 + 6) // 7, clearance=False)
            joints(b"belongs to another context", tree=foreign._handle_or_raise())
            from_poses(b"null", link_poses=None)
            from_poses(b"the joint gradient needs the kinematic tree", tree=None)
            from_poses(b"the kinematic tree has 8 links, the poses have 9", links=9)
            from_poses(b"the kinematic tree has 15 links, the poses have 8", tree=body._handle_or_raise())
            from_poses(b"at least one link", tree=None, links=0, gradient=False)
            from_poses(b"must not be negative", tree=None, links=-1, gradient=False)
            from_poses(b"unknown self-collision flag", flags=4)
            from_poses(b"minimum_clearance must not be NaN", minimum=np.nan)
            if host:
                bad = link.copy()
                bad[1], bad[3] = t.num_links, -1
                joints(b"sphere 1: link 8 is not in [0, num_links)", link=bad)
                from_poses(b"sphere 1: link 8 is not in [0, num_links)", link=bad)
                radius = xyzr.copy()
                radius[2, 3], radius[4, 3] = -0.5, np.nan
                joints(b"sphere 2: the radius must not be negative or NaN", xyzr=radius)
                for rows, needle in (([[0, 1], [1, 5], [7, 2]], b"pair 1: sphere 5 is outside [0, 5)"),
                                     ([[0, 1], [-1, 3], [2, 2]], b"pair 1: sphere -1 is outside [0, 5)"),
                                     ([[0, 1], [1, 2], [3, 3], [4, 1]], b"pair 2: (3, 3) is not ascending"),
                                     ([[0, 1], [1, 2], [3, 4], [4, 1]], b"pair 3: (4, 1) is not ascending")):
                    listed = np.zeros((4, 2), np.int32)
                    listed[:len(rows)] = rows
                    listed[len(rows):] = [0, 1]
                    joints(needle, pairs=listed)
                    from_poses(needle, pairs=listed)
        for o in outputs:
            assert (o == 9).all()
    other.close()
    # no configurations: success without a device, whatever the tree
    assert lib.vgt_hip_check_self_collision(ctx.handle, None, None, 0, None, 0, None, None, 0, None, None, 0.0, 0,
                                            capi._ptr(outputs[0]), *([None] * 8)) == 1      # (the tree is required)
    with make_tree(ctx, t) as tree:
        assert lib.vgt_hip_check_self_collision(ctx.handle, capi._ptr(xyzr), capi._ptr(link), 5, capi._ptr(pairs), 4,
                                                tree._handle_or_raise(), None, 0, None, None, 0.0, 0,
                                                capi._ptr(outputs[0]), *([None] * 8)) == 0
    assert (outputs[0] == 9).all()
