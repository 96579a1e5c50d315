"""(gpu) vgt_hip_check_motions_with_self[_dev] against tests/motion_self_ref.py, the CPU restatement: every output
bit-equal (NaNs by position) on the shared cases of tests/motion_self_cases.py, with and without
VGT_HIP_MOTION_STOP_AT_COLLISION -- through the host form of the product library, and the device form on torch buffers
through the testing library limited to one and to three workgroups, so that the persistent waves stride, and with the
default.  Then the tile query, models on both sides of the refusal limit, pair lists of every length around the lanes of a
sample, the calls that exist without this one, the call without a self part against vgt_hip_check_motions_dev, the
field-less form, in the device form an invalid step count, links and sphere indices out of range and a model without
spheres, outputs passed as NULL, and the argument errors that need a tree or a context."""
import functools

import numpy as np
import pytest

import kinematics_cases
import motion_ref
import motion_self_cases as C
import motion_self_ref as R
import self_ref
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu

FIELDS = capi.MotionSelfChecks._fields
GUARD = 16
OUTPUTS = (("status", 1, "uint8"), ("first_collision", 1, "int32"), ("collision_cause", 1, "uint8"),
           ("min_clearance", 1, "float64"), ("min_sample", 1, "int32"), ("min_sphere", 1, "int32"),
           ("min_gradient", 3, "float64"), ("self_min_clearance", 1, "float64"), ("self_min_sample", 1, "int32"),
           ("self_min_pair", 1, "int32"), ("fk_status", 1, "uint8"))


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def testing_ctx():
    c = capi.Context(0, testing=True)
    yield c
    c.set_motion_self_workgroups(0)
    c.set_motion_workgroups(0)
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
        if not same_bits(g, w):
            rows = np.flatnonzero([not same_bits(g[e], w[e]) for e in range(len(w))])
            raise AssertionError("%s: %s differs in motions %s: got %s, want %s"
                                 % (what, name, rows[:8].tolist(), g[rows[:3]].tolist(), w[rows[:3]].tolist()))


def host_form(context, tree, case, stop):
    return context.check_motions_with_self(
        case.sdf, C.RESOLUTION, case.xyzr, case.link, case.pairs, tree, case.joint_from, case.joint_to, case.num_steps,
        case.minimum_clearance, case.self_minimum_clearance, case.outside_is_collision, stop,
        case.self_no_value_is_collision, grid_from_world=case.grid_from_world, rotation=case.rotation,
        world_from_base=case.world_from_base, joint_limits=case.joint_limits)


def _on_device(array, stand_in):
    import torch
    array = np.asarray(array)
    return torch.from_numpy(np.array(array if array.size else stand_in)).cuda()     # (copies: the cases are read-only)


def device_form(context, tree, case, stop, without=(), num_steps=None, num_spheres=None, num_pairs=None):
    """The device form on torch buffers filled with 77, GUARD elements behind each output -> MotionSelfChecks; the
    outputs named in `without` are passed as NULL and come back as they were.  Asserts that the guards are untouched."""
    import torch
    motions = len(case.joint_from)
    steps = case.num_steps if num_steps is None else num_steps
    sdf = None if case.sdf is None else torch.from_numpy(np.array(case.sdf)).cuda()     # (copies: read-only)
    xyzr = _on_device(case.xyzr, np.zeros((1, 4)))         # (torch has no pointer for an empty tensor: one element stands in)
    link = _on_device(case.link, np.zeros(1, np.int32))
    pairs = _on_device(case.pairs, np.zeros((1, 2), np.int32))
    joint_from = _on_device(case.joint_from, np.zeros(1))
    joint_to = _on_device(case.joint_to, np.zeros(1))
    steps_dev = None if np.ndim(steps) == 0 else torch.from_numpy(np.ascontiguousarray(steps, dtype=np.int32)).cuda()
    out = {name: torch.full((motions * width + GUARD,), 77, dtype=getattr(torch, dtype), device="cuda")
           for name, width, dtype in OUTPUTS}
    torch.cuda.synchronize()
    pointers = {name + "_ptr": None if name in without else out[name].data_ptr() for name in out if name != "status"}
    context.check_motions_with_self_dev(
        None if sdf is None else sdf.data_ptr(), (0, 0, 0) if sdf is None else case.sdf.shape, C.RESOLUTION,
        xyzr.data_ptr(), link.data_ptr(), len(case.link) if num_spheres is None else num_spheres, pairs.data_ptr(),
        len(case.pairs) if num_pairs is None else num_pairs, tree, joint_from.data_ptr(), joint_to.data_ptr(),
        int(steps) if steps_dev is None else 0, motions, out["status"].data_ptr(),
        minimum_clearance=case.minimum_clearance, self_minimum_clearance=case.self_minimum_clearance,
        outside_is_collision=case.outside_is_collision, stop_at_collision=stop,
        self_no_value_is_collision=case.self_no_value_is_collision, grid_from_world=case.grid_from_world,
        rotation=case.rotation, world_from_base=case.world_from_base, joint_limits=case.joint_limits,
        num_steps_ptr=None if steps_dev is None else steps_dev.data_ptr(), **pointers)
    context.synchronize()
    got = []
    for name, width, _ in OUTPUTS:
        flat = out[name].cpu().numpy()
        assert (flat[motions * width:] == 77).all(), "the guard behind %s" % name
        flat = flat[:motions * width]
        got.append(flat.reshape(motions, 3) if width == 3 else flat)
    return capi.MotionSelfChecks(*got)


def report(case, got):
    print(case.name, "P", len(case.pairs), "statuses", np.bincount(got.status, minlength=4).tolist(), "causes",
          np.bincount(got.collision_cause, minlength=4).tolist(), "tile",
          capi.motion_self_tile_samples(case.tree.num_links, len(case.link)))


def test_tile_query_is_what_the_header_says():
    for links, spheres in [(1, 0), (1, 21), (8, 16), (8, 21), (15, 9), (8, 64), (8, 70), (8, 200), (15, 200), (8, 257),
                           (18, 21), (84, 6), (85, 6), (664, 0), (665, 0), (1, 1989), (1, 1990), (0, 5), (-1, 5), (5, -1),
                           (2 ** 40, 1), (1, 2 ** 40)]:
        assert capi.motion_self_tile_samples(links, spheres) == C.tile_formula(links, spheres), (links, spheres)
    assert capi.motion_self_tile_samples(8, 21) == 8             # (what the pair counts below sit around)
    assert capi.motion_self_tile_samples(664, 0) == 1 and capi.motion_self_tile_samples(1, 1989) == 1


@pytest.mark.parametrize("stop", [False, True], ids=["all", "stop"])
@pytest.mark.parametrize("index", range(len(C.names())), ids=C.names())
def test_host_form(ctx, index, stop):
    case = C.case(index)
    with make_tree(ctx, case.tree) as tree:
        got = host_form(ctx, tree, case, stop)
    report(case, got)
    assert_same(got, case.want_stopped if stop else case.want, case.name)


@pytest.mark.parametrize("workgroups", [1, 3, 0])
@pytest.mark.parametrize("stop", [False, True], ids=["all", "stop"])
@pytest.mark.parametrize("index", range(len(C.names())), ids=C.names())
def test_device_form_with_striding_waves(testing_ctx, index, stop, workgroups):
    case = C.case(index)
    testing_ctx.set_motion_self_workgroups(workgroups)
    with make_tree(testing_ctx, case.tree) as tree:
        got = device_form(testing_ctx, tree, case, stop)
    assert_same(got, case.want_stopped if stop else case.want, case.name)


def test_device_form_of_the_product_library(ctx):
    case = C.case(C.names().index("body-9"))
    with make_tree(ctx, case.tree) as tree:
        assert_same(device_form(ctx, tree, case, False), case.want, case.name)
        assert_same(device_form(ctx, tree, case, True), case.want_stopped, case.name)


def test_models_on_both_sides_of_the_refusal_limit(ctx):
    """1989 spheres on one link run, with a field and without one; 1990 are refused; a chain of 665 links is refused."""
    from oracle import oracle as O
    import body_cases
    t = kinematics_cases.tree("fixed1")
    xyzr, link = kinematics_cases.sphere_model(t, 1990, 5)
    pairs = np.array([[0, 1988], [5, 1987], [1987, 1988], [7, 1000], [1, 2]], np.int32)
    none = np.zeros((3, 0))
    sdf = body_cases.field(False)
    base = C.motion_cases.world_from_base()
    with make_tree(ctx, t) as tree:
        for field in (sdf, None):
            want = R.check_motions_with_self(O, field, C.RESOLUTION, xyzr[:1989], link[:1989], pairs, t, none, none, 2,
                                             self_minimum_clearance=-0.05, world_from_base=base)
            got = ctx.check_motions_with_self(field, C.RESOLUTION, xyzr[:1989], link[:1989], pairs, tree, none, none, 2,
                                              self_minimum_clearance=-0.05, world_from_base=base)
            assert_same(got, want, "1989 spheres")
            assert np.isfinite(got.self_min_clearance).all() and (got.self_min_sample == 0).all()
        with pytest.raises(ValueError, match="this model has 1 links and 1990 spheres"):
            ctx.check_motions_with_self(sdf, C.RESOLUTION, xyzr, link, pairs, tree, none, none, 2)
    t = kinematics_cases.tree("chain-665")
    with make_tree(ctx, t) as tree:
        with pytest.raises(ValueError, match="this model has 665 links and 2 spheres"):
            ctx.check_motions_with_self(sdf, C.RESOLUTION, xyzr[:2], [0, 664], [[0, 1]], tree,
                                        np.zeros((1, t.num_joints)), np.zeros((1, t.num_joints)), 2)


@functools.lru_cache(maxsize=None)
def _shortened(num_pairs):
    """arm-21 with the first num_pairs entries of its list turned round, so that the worst pairs come early."""
    case = C.case(C.names().index("arm-21"))
    pairs = np.ascontiguousarray(case.pairs[::-1][:num_pairs])
    q, first = motion_ref.interpolate(case.joint_from, case.joint_to, case.num_steps)
    own = R.check_self_samples(case.xyzr, case.link, pairs, case.tree, q, case.self_minimum_clearance,
                               case.self_no_value_is_collision, case.world_from_base, case.joint_limits)
    return case._replace(pairs=pairs, name="arm-21-P%d" % num_pairs, self_samples=own,
                         want=R.reduce_with_self(case.samples, own, first, False),
                         want_stopped=R.reduce_with_self(case.samples, own, first, True))


def pair_counts():
    per_sample = 64 // C.tile_formula(8, 21)
    return sorted({1, per_sample - 1, per_sample, per_sample + 1, 2 * per_sample + 1})


@pytest.mark.parametrize("num_pairs", pair_counts())
def test_pair_lists_around_the_lanes_of_a_sample(ctx, testing_ctx, num_pairs):
    case = _shortened(num_pairs)
    assert len(case.pairs) == num_pairs
    testing_ctx.set_motion_self_workgroups(3)
    with make_tree(testing_ctx, case.tree) as tree:
        for stop in (False, True):
            got = device_form(testing_ctx, tree, case, stop)
            assert_same(got, case.want_stopped if stop else case.want, case.name)
    report(case, got)
    with make_tree(ctx, case.tree) as tree:
        assert_same(host_form(ctx, tree, case, False), case.want, case.name)


def _flat_self_checks(context, tree, case, q):
    """vgt_hip_check_self_collision_dev on the flat samples -> (status, min_clearance, min_pair, fk_status)."""
    import torch
    num = len(q)
    dev = [_on_device(a, s) for a, s in ((case.xyzr, np.zeros((1, 4))), (case.link, np.zeros(1, np.int32)),
                                         (case.pairs, np.zeros((1, 2), np.int32)), (q, np.zeros(1)))]
    status = torch.zeros(num, dtype=torch.uint8, device="cuda")
    clearance = torch.zeros(num, dtype=torch.float64, device="cuda")
    pair = torch.zeros(num, dtype=torch.int32, device="cuda")
    fk_status = torch.zeros(num, dtype=torch.uint8, device="cuda")
    context.check_self_collision_dev(dev[0].data_ptr(), dev[1].data_ptr(), len(case.link), dev[2].data_ptr(),
                                     len(case.pairs), tree, dev[3].data_ptr(), num, status.data_ptr(),
                                     minimum_clearance=case.self_minimum_clearance, min_clearance_ptr=clearance.data_ptr(),
                                     min_pair_ptr=pair.data_ptr(), fk_status_ptr=fk_status.data_ptr(),
                                     world_from_base=case.world_from_base, joint_limits=case.joint_limits,
                                     flags=int(case.self_no_value_is_collision))
    context.synchronize()
    return [t.cpu().numpy() for t in (status, clearance, pair, fk_status)]


def _motions_alone(context, tree, case, stop):
    """vgt_hip_check_motions_dev on the case -> motion_ref.MotionChecks."""
    import torch
    motions = len(case.joint_from)
    dev = [_on_device(a, s) for a, s in ((case.sdf, None), (case.xyzr, np.zeros((1, 4))),
                                         (case.link, np.zeros(1, np.int32)), (case.joint_from, np.zeros(1)),
                                         (case.joint_to, np.zeros(1)))]
    steps = case.num_steps
    steps_dev = None if np.ndim(steps) == 0 else torch.from_numpy(np.ascontiguousarray(steps, dtype=np.int32)).cuda()
    kinds = (("status", 1, "uint8"), ("first_collision", 1, "int32"), ("min_clearance", 1, "float64"),
             ("min_sample", 1, "int32"), ("min_sphere", 1, "int32"), ("min_gradient", 3, "float64"),
             ("fk_status", 1, "uint8"))
    out = {name: torch.full((motions * width,), 77, dtype=getattr(torch, dtype), device="cuda")
           for name, width, dtype in kinds}
    pointers = {name + "_ptr": out[name].data_ptr() for name in out if name != "status"}
    context.check_motions_dev(dev[0].data_ptr(), case.sdf.shape, C.RESOLUTION, dev[1].data_ptr(), dev[2].data_ptr(),
                              len(case.link), tree, dev[3].data_ptr(), dev[4].data_ptr(),
                              int(steps) if steps_dev is None else 0, motions, out["status"].data_ptr(),
                              minimum_clearance=case.minimum_clearance, outside_is_collision=case.outside_is_collision,
                              stop_at_collision=stop, grid_from_world=case.grid_from_world, rotation=case.rotation,
                              world_from_base=case.world_from_base, joint_limits=case.joint_limits,
                              num_steps_ptr=None if steps_dev is None else steps_dev.data_ptr(), **pointers)
    context.synchronize()
    got = [out[name].cpu().numpy() for name, _, _ in kinds]
    got[5] = got[5].reshape(motions, 3)
    return motion_ref.MotionChecks(*got)


@pytest.mark.parametrize("name", ["arm-21", "body-9-odd"])
def test_equals_the_calls_that_exist_without_it(ctx, name):
    """The route a caller had to take: the samples interpolated on the host, vgt_hip_check_motions_dev for the
    environment's verdict per motion, vgt_hip_check_self_collision_dev on the flat samples, and the two combined per
    motion in numpy.  Without the stop flag that route gives every output of the call.  (It cannot stop across the two
    checks; with the stop flag the environment part per sample comes from check_spheres_from_joints and the reduction is
    the restatement's.)  This holds the kernel's restated pair arithmetic to self_collision_kernels.hip's."""
    case = C.case(C.names().index(name))
    q, first = motion_ref.interpolate(case.joint_from, case.joint_to, case.num_steps)
    with make_tree(ctx, case.tree) as tree:
        got = device_form(ctx, tree, case, False)
        stopped = device_form(ctx, tree, case, True)
        alone = _motions_alone(ctx, tree, case, False)
        status, clearance, pair, fk_status = _flat_self_checks(ctx, tree, case, q)
        flat = ctx.check_spheres_from_joints(case.sdf, C.RESOLUTION, case.xyzr, case.link, tree, q,
                                             minimum_clearance=case.minimum_clearance,
                                             outside_is_collision=case.outside_is_collision,
                                             grid_from_world=case.grid_from_world, rotation=case.rotation,
                                             world_from_base=case.world_from_base, joint_limits=case.joint_limits)
    motions = len(first) - 1
    for e in range(motions):
        lo, hi = int(first[e]), int(first[e + 1])
        hits = np.flatnonzero(status[lo:hi] == capi.SELF_COLLISION)
        own = int(hits[0]) if len(hits) else -1
        theirs = int(alone.first_collision[e])
        both = [k for k in (own, theirs) if k >= 0]
        want_first = min(both) if both else -1
        want_cause = (1 if theirs == want_first else 0) | (2 if own == want_first else 0) if both else 0
        want_status = (capi.MOTION_COLLISION if both else capi.MOTION_NO_VALUE
                       if alone.status[e] == capi.MOTION_NO_VALUE or (status[lo:hi] == capi.SELF_NO_VALUE).any()
                       else capi.MOTION_CLEAR)
        assert (got.status[e], got.first_collision[e], got.collision_cause[e]) == (want_status, want_first, want_cause), e
        values = clearance[lo:hi]
        k = -1
        if not np.isnan(values).all():
            k = int(np.flatnonzero(values == np.nanmin(values))[0])
        assert got.self_min_sample[e] == k and got.self_min_pair[e] == (pair[lo + k] if k >= 0 else -1), e
        assert same_bits(got.self_min_clearance[e], values[k] if k >= 0 else np.float64(np.nan)), e
        assert got.fk_status[e] == np.bitwise_or.reduce(fk_status[lo:hi]) == alone.fk_status[e], e
    for field in R.ENVIRONMENT:
        assert same_bits(getattr(got, field), getattr(alone, field)), field
    samples = motion_ref.Samples(flat.status, flat.min_clearance, flat.min_sphere, flat.min_gradient, flat.fk_status)
    own = self_ref.SelfCollisionChecks(status, None, None, clearance, pair, None, None, fk_status, None)
    assert_same(got, R.reduce_with_self(samples, own, first, False), name)
    assert_same(stopped, R.reduce_with_self(samples, own, first, True), name + " with the stop flag")


@pytest.mark.parametrize("name", ["arm-21", "body-9-odd", "arm-257", C.names()[7]])
def test_without_the_self_part_it_is_check_motions(testing_ctx, name):
    """P == 0: every output the two calls share is vgt_hip_check_motions_dev's to the bit, with and without the stop flag;
    the cause is 1 where there is a collision and the self outputs say that there is none."""
    case = C.case(C.names().index(name))
    bare = case._replace(pairs=np.zeros((0, 2), np.int32))
    testing_ctx.set_motion_self_workgroups(3)
    with make_tree(testing_ctx, case.tree) as tree:
        for stop in (False, True):
            got = device_form(testing_ctx, tree, bare, stop)
            want = _motions_alone(testing_ctx, tree, case, stop)
            for field in R.SHARED:
                assert same_bits(getattr(got, field), getattr(want, field)), (name, stop, field)
            assert np.array_equal(got.collision_cause, (want.first_collision >= 0).astype(np.uint8))
            assert np.isnan(got.self_min_clearance).all() and (got.self_min_sample == -1).all()
            assert (got.self_min_pair == -1).all()
        assert (want.first_collision >= 0).any()
        # the host form too
        host = host_form(testing_ctx, tree, bare, True)
        for field in R.SHARED:
            assert same_bits(getattr(host, field), getattr(want, field)), (name, field)


def test_without_the_stop_flag_the_environment_outputs_are_those_of_check_motions(ctx):
    case = C.case(C.names().index("arm-70"))
    with make_tree(ctx, case.tree) as tree:
        got = device_form(ctx, tree, case, False)
        alone = _motions_alone(ctx, tree, case, False)
    for field in R.ENVIRONMENT:
        assert same_bits(getattr(got, field), getattr(alone, field)), field
    assert (got.first_collision != alone.first_collision).sum() >= 3


def test_the_field_less_form(ctx, testing_ctx):
    """No field: the environment outputs say so, whatever extents and field arguments are passed along."""
    case = C.case(C.names().index("arm-21-field-less"))
    assert case.sdf is None
    with make_tree(ctx, case.tree) as tree:
        for stop in (False, True):
            got = host_form(ctx, tree, case, stop)
            assert_same(got, case.want_stopped if stop else case.want, case.name)
            assert np.isnan(got.min_clearance).all() and np.isnan(got.min_gradient).all()
            assert (got.min_sample == -1).all() and (got.min_sphere == -1).all()
            assert not (got.collision_cause & capi.MOTION_CAUSE_ENVIRONMENT).any()
        report(case, got)
        assert set(got.status.tolist()) == {capi.MOTION_CLEAR, capi.MOTION_COLLISION, capi.MOTION_NO_VALUE}
    # a case with a field, its field taken away: the self part's verdict alone
    case = C.case(C.names().index("body-9"))
    bare = case._replace(sdf=None, grid_from_world=None, rotation=None)
    testing_ctx.set_motion_self_workgroups(3)
    with make_tree(testing_ctx, case.tree) as tree:
        for stop in (False, True):
            want = R.reduce_with_self(None, case.self_samples, case.first, stop)
            assert_same(device_form(testing_ctx, tree, bare, stop), want, "body-9 without its field")


def test_a_negative_step_count_in_the_device_form(testing_ctx):
    case = C.case(C.names().index("arm-21"))
    steps = np.array(case.num_steps, dtype=np.int32)
    steps[[0, 11, 66]] = [-1, -7, -2147483648]
    testing_ctx.set_motion_self_workgroups(2)
    with make_tree(testing_ctx, case.tree) as tree:
        got = device_form(testing_ctx, tree, case, False, num_steps=steps)
    invalid = steps < 0
    assert (got.status[invalid] == capi.MOTION_INVALID).all() and (got.first_collision[invalid] == -1).all()
    assert (got.collision_cause[invalid] == 0).all() and (got.fk_status[invalid] == 0).all()
    assert np.isnan(got.min_clearance[invalid]).all() and np.isnan(got.min_gradient[invalid]).all()
    assert (got.min_sample[invalid] == -1).all() and (got.min_sphere[invalid] == -1).all()
    assert np.isnan(got.self_min_clearance[invalid]).all()
    assert (got.self_min_sample[invalid] == -1).all() and (got.self_min_pair[invalid] == -1).all()
    for name in FIELDS:
        assert same_bits(getattr(got, name)[~invalid], getattr(case.want, name)[~invalid]), name


@pytest.mark.parametrize("stop", [False, True], ids=["all", "stop"])
def test_device_form_with_links_and_spheres_out_of_range(testing_ctx, stop):
    """The device form cannot look at the model or the list: a sphere whose link is outside [0, L) is "without a value"
    for both parts, a pair with a sphere outside [0, S) too (the restatements' rules), and no address is formed from
    either.  Then fewer spheres than the list knows."""
    from oracle import oracle as O
    case = C.case(C.names().index("arm-21"))
    count = len(case.link)
    link = np.array(case.link)
    link[[2, 9, 20]] = [case.tree.num_links, -1, 2 ** 31 - 1]
    pairs = np.array(case.pairs)
    pairs[[1, 7, 20, 33]] = [[-1, 3], [4, count], [2 ** 31 - 1, 5], [-2 ** 31, 2 ** 31 - 1]]
    for changed, spheres in ((case._replace(link=link, pairs=pairs), count), (case, 10)):
        want = R.check_motions_with_self(
            O, case.sdf, C.RESOLUTION, changed.xyzr[:spheres], changed.link[:spheres], changed.pairs, case.tree,
            case.joint_from, case.joint_to, case.num_steps, case.minimum_clearance, case.self_minimum_clearance,
            case.outside_is_collision, stop, case.self_no_value_is_collision, world_from_base=case.world_from_base,
            joint_limits=case.joint_limits)
        for workgroups in (1, 0):
            testing_ctx.set_motion_self_workgroups(workgroups)
            with make_tree(testing_ctx, case.tree) as tree:
                got = device_form(testing_ctx, tree, changed, stop, num_spheres=spheres)
            assert_same(got, want, "arm-21 out of range, %d spheres" % spheres)
    assert (want.status == capi.MOTION_COLLISION).any()


@pytest.mark.parametrize("stop", [False, True], ids=["all", "stop"])
def test_a_model_without_spheres(ctx, testing_ctx, stop):
    """S == 0: the pair list is not looked at in either form (its one pair names spheres that do not exist, and in the
    device form the pointer may be anything); every sample is NO_VALUE in both parts, the kinematics status is there."""
    case = C.case(C.names().index("arm-0"))
    want = case.want_stopped if stop else case.want
    with make_tree(ctx, case.tree) as tree:
        assert_same(host_form(ctx, tree, case, stop), want, case.name)
    with make_tree(testing_ctx, case.tree) as tree:
        got = device_form(testing_ctx, tree, case, stop)
    assert_same(got, want, case.name)
    assert (got.status == capi.MOTION_NO_VALUE).all() and (got.min_sample == -1).all() and got.fk_status.any()
    assert (got.self_min_sample == -1).all() and (got.collision_cause == 0).all()


def test_outputs_passed_as_null_stay_untouched(testing_ctx):
    case = C.case(C.names().index("body-9-odd"))
    optional = [name for name, _, _ in OUTPUTS if name != "status"]
    some_names = ("min_clearance", "min_gradient", "fk_status", "self_min_pair", "collision_cause")
    other_names = ("first_collision", "min_sample", "min_sphere", "self_min_clearance", "self_min_sample")
    testing_ctx.set_motion_self_workgroups(2)
    with make_tree(testing_ctx, case.tree) as tree:
        none = device_form(testing_ctx, tree, case, False, without=optional)
        some = device_form(testing_ctx, tree, case, True, without=some_names)
        other = device_form(testing_ctx, tree, case, False, without=other_names)
    assert same_bits(none.status, case.want.status)
    for name in optional:
        assert (getattr(none, name) == 77).all(), name
    for got, want, names in ((some, case.want_stopped, some_names), (other, case.want, other_names)):
        for name in FIELDS:
            if name in names:
                assert (getattr(got, name) == 77).all(), name
            else:
                assert same_bits(getattr(got, name), getattr(want, name)), name


def test_argument_errors_that_need_a_tree_or_a_context(ctx):
    """Through the C ABI itself, both forms: each is VGT_HIP_ERR_INVALID_ARGUMENT with its message, before any device
    work: the arrays behind the pointers are small host arrays that no rejected call may touch, and the outputs stay as
    they were."""
    import body_cases
    lib = ctx._lib
    t = kinematics_cases.tree("arm")                       # L = 8, J = 7
    sdf = body_cases.field(False)
    xyzr, link = kinematics_cases.sphere_model(t, 5, 31)
    xyzr, link = np.ascontiguousarray(xyzr), np.ascontiguousarray(link)
    pairs = np.array([[0, 1], [1, 4], [2, 3], [0, 4]], np.int32)
    a, b = np.zeros((3, t.num_joints)), np.ones((3, t.num_joints))
    outputs = [np.full(3, 9, np.uint8), np.full(3, 9, np.int32), np.full(3, 9, np.uint8), np.full(3, 9.0),
               np.full(3, 9, np.int32), np.full(3, 9, np.int32), np.full((3, 3), 9.0), np.full(3, 9.0),
               np.full(3, 9, np.int32), np.full(3, 9, np.int32), np.full(3, 9, np.uint8)]
    other = capi.Context(0)
    with make_tree(ctx, t) as tree, make_tree(other, t) as foreign:
        handle = tree._handle_or_raise()
        for host, fn in ((True, lib.vgt_hip_check_motions_with_self), (False, lib.vgt_hip_check_motions_with_self_dev)):
            def refused(needle, link=link, pairs=pairs, a=capi._ptr(a), b=capi._ptr(b), motions=3, tree=handle,
                        field=capi._ptr(sdf), num_pairs=4):
                rc = fn(ctx.handle, field, *sdf.shape, C.RESOLUTION, None, None, capi._ptr(xyzr), capi._ptr(link),
                        len(xyzr), capi._ptr(pairs), num_pairs, tree, a, b, None, 2, motions, None, None, 0.0, 0.0, 0,
                        *[capi._ptr(o) for o in outputs])
                message = lib.vgt_hip_last_error()
                assert rc == 1 and needle in message, (host, rc, message)

            refused(b"null", a=None)
            refused(b"null", b=None)
            refused(b"null", pairs=None)
            refused(b"neither a field nor a pair", field=None, num_pairs=0)
            refused(b"2^31 (motion, joint) pairs", motions=2 ** 30)            # 2^30 * 7 >= 2^31
            refused(b"2^31 (motion, joint) pairs", motions=(2 ** 31 + 6) // 7)  # the least such E
            refused(b"belongs to another context", tree=foreign._handle_or_raise())
            if host:
                for first, second in ((t.num_links, -1), (-1, t.num_links), (2 ** 31 - 1, -1)):
                    bad = link.copy()
                    bad[1], bad[3] = first, second
                    refused(b"sphere 1: link %d is not in [0, num_links)" % first, link=bad)
                for rows, needle in (([[0, 1], [1, 5], [7, 2]], b"pair 1: sphere 5 is outside [0, 5)"),
                                     ([[0, 1], [1, 2], [3, 3], [4, 1]], b"pair 2: (3, 3) is not ascending")):
                    listed = np.zeros((4, 2), np.int32)
                    listed[:len(rows)] = rows
                    listed[len(rows):] = [0, 1]
                    refused(needle, pairs=listed)
        for o in outputs:
            assert (o == 9).all()
    other.close()
