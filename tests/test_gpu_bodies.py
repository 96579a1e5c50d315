"""(gpu) vgt_hip_check_spheres[_dev] against tests/body_ref.py, the CPU restatement of the call: every output bit-equal
(NaNs by position), through the host entry point of the product library and through the device entry point on torch
buffers -- the latter through the testing library with the launch limited to two workgroups, so that the shared cases'
67 and 257 configurations make the kernel's persistent waves take several trips -- on the shapes of tests/body_cases.py."""
import numpy as np
import pytest

import body_cases as C
import body_ref as R
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu

FIELDS = R.SphereChecks._fields


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def few_workgroups():
    """A context of the testing library whose sphere-model launches have at most two workgroups (eight waves)."""
    c = capi.Context(0, testing=True)
    c.set_check_spheres_workgroups(2)
    yield c
    c.set_check_spheres_workgroups(0)
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return np.array_equal(nan_a, nan_b) and np.array_equal(a[~nan_a].view(np.uint64), b[~nan_b].view(np.uint64))


def assert_same(got, want, what, per_sphere=True):
    print(what, "statuses", np.bincount(got.status, minlength=3).tolist(), "below", int(got.num_below.sum()), "outside",
          int(got.num_outside.sum()))
    for name in FIELDS:
        g, w = getattr(got, name), getattr(want, name)
        if name.startswith("sphere_") and not per_sphere:
            assert g is None, name
            continue
        assert g is not None and same_bits(g, w), (what, name)


def check_dev(ctx, case, leave_out=(), xyzr=None, link=None):
    """The device-pointer entry point on torch buffers; `leave_out`: outputs passed as NULL (returned as None)."""
    import torch
    xyzr = case.xyzr if xyzr is None else xyzr
    link = case.link if link is None else link
    b, links, s = case.poses.shape[0], case.poses.shape[1], len(xyzr)
    dev = {"sdf": torch.from_numpy(np.ascontiguousarray(case.sdf)).cuda(),
           "xyzr": torch.from_numpy(np.ascontiguousarray(xyzr)).cuda(),
           "link": torch.from_numpy(np.ascontiguousarray(link, dtype=np.int32)).cuda(),
           "poses": torch.from_numpy(np.ascontiguousarray(case.poses)).cuda()}
    shapes = {"status": ((b,), torch.uint8), "min_clearance": ((b,), torch.float64), "min_sphere": ((b,), torch.int32),
              "num_below": ((b,), torch.int32), "num_outside": ((b,), torch.int32), "min_gradient": ((b, 3), torch.float64),
              "sphere_clearance": ((b, s), torch.float64), "sphere_gradient": ((b, s, 3), torch.float64)}
    out = {name: torch.full(shape, 77, dtype=dtype, device="cuda") for name, (shape, dtype) in shapes.items()
           if name not in leave_out}
    torch.cuda.synchronize()
    ctx.check_spheres_dev(dev["sdf"].data_ptr(), case.sdf.shape, case.resolution, dev["xyzr"].data_ptr(),
                          dev["link"].data_ptr(), s, dev["poses"].data_ptr(), links, b, out["status"].data_ptr(),
                          **{name + "_ptr": t.data_ptr() for name, t in out.items() if name != "status"},
                          minimum_clearance=case.minimum_clearance, outside_is_collision=case.outside_is_collision,
                          grid_from_world=case.grid_from_world, rotation=case.rotation)
    ctx.synchronize()
    return R.SphereChecks(*[out[name].cpu().numpy() if name in out else None for name in FIELDS])


@pytest.mark.parametrize("index", range(len(C.SHAPES)), ids=C.names())
def test_host_form(ctx, index):
    case = C.case(index)
    got = ctx.check_spheres(case.sdf, case.resolution, case.xyzr, case.link, case.poses, case.minimum_clearance,
                            case.outside_is_collision, per_sphere=True, grid_from_world=case.grid_from_world,
                            rotation=case.rotation)
    assert_same(got, case.want, case.name + " (host)")


@pytest.mark.parametrize("index", range(len(C.SHAPES)), ids=C.names())
def test_device_form_with_striding_waves(few_workgroups, index):
    case = C.case(index)
    assert_same(check_dev(few_workgroups, case), case.want, case.name + " (dev, 2 workgroups)")


def test_device_form_of_the_product_library(ctx):
    for index in (2, 12, 21):
        case = C.case(index)
        assert_same(check_dev(ctx, case), case.want, case.name + " (dev)")


def test_four_by_four_poses_and_no_per_sphere_outputs(ctx):
    case = C.case(9)
    b, links = case.poses.shape[:2]
    matrices = case.poses.reshape(b, links, 4, 4).transpose(0, 1, 3, 2)              # world_from_link as matrices
    got = ctx.check_spheres(case.sdf, case.resolution, case.xyzr, case.link, matrices, case.minimum_clearance,
                            case.outside_is_collision, grid_from_world=case.grid_from_world, rotation=case.rotation)
    assert_same(got, case.want, case.name + " (4 x 4)", per_sphere=False)


@pytest.mark.parametrize("index", [6, 20], ids=["S3-L3-B67", "S130-L7-B67"])
def test_optional_outputs_left_out_one_at_a_time(few_workgroups, index):
    case = C.case(index)
    for name in FIELDS[1:]:
        got = check_dev(few_workgroups, case, leave_out=(name,))
        for other in FIELDS:
            if other == name:
                assert getattr(got, other) is None
            else:
                assert same_bits(getattr(got, other), getattr(case.want, other)), (name, other)
    only_status = check_dev(few_workgroups, case, leave_out=FIELDS[1:])
    assert same_bits(only_status.status, case.want.status)


@pytest.mark.parametrize("index", range(len(C.SHAPES)), ids=C.names())
def test_per_sphere_outputs_agree_with_the_per_configuration_ones(ctx, index):
    """On the device's own outputs, without the restatement."""
    case = C.case(index)
    got = ctx.check_spheres(case.sdf, case.resolution, case.xyzr, case.link, case.poses, case.minimum_clearance,
                            case.outside_is_collision, per_sphere=True, grid_from_world=case.grid_from_world,
                            rotation=case.rotation)
    clearance, gradient = got.sphere_clearance, got.sphere_gradient
    # a sphere without a value has a NaN clearance and a NaN gradient; on the fields without odd cells only such a sphere
    without = np.sum(np.isnan(clearance) & np.isnan(gradient).all(axis=2), axis=1)
    assert (got.num_outside <= without).all() and (index % 3 == 2 or np.array_equal(got.num_outside, without))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(got.num_below, np.sum(clearance <= case.minimum_clearance, axis=1))
    for b in range(len(got.status)):
        k = got.min_sphere[b]
        if k < 0:
            assert np.isnan(clearance[b]).all() and np.isnan(got.min_clearance[b]) and np.isnan(got.min_gradient[b]).all()
            continue
        assert same_bits(got.min_clearance[b:b + 1], clearance[b, k:k + 1])
        assert same_bits(got.min_gradient[b], gradient[b, k])
        assert not (clearance[b] < clearance[b, k]).any() and not (clearance[b, :k] == clearance[b, k]).any()
    collision = (got.num_below > 0) | (case.outside_is_collision & (got.num_outside > 0))
    assert np.array_equal(got.status, np.where(collision, 1, np.where(got.min_sphere >= 0, 0, 2)))


def test_a_link_out_of_range_through_the_device_form_is_a_sphere_without_a_value(few_workgroups):
    from oracle import oracle as O
    case = C.case(12)                                                               # S = 33, L = 3
    link = case.link.copy()
    link[[0, 7, 32]] = [3, -1, 2 ** 31 - 1]
    want = R.check_spheres(O, case.sdf, case.resolution, case.xyzr, link, case.poses, case.minimum_clearance,
                           case.outside_is_collision, case.grid_from_world, case.rotation)
    assert (want.num_outside >= 3).all() and np.isnan(want.sphere_clearance[:, [0, 7, 32]]).all()
    assert_same(check_dev(few_workgroups, case, link=link), want, case.name + " (links out of range)")
    with pytest.raises(ValueError, match="sphere 0: link 3"):
        few_workgroups.check_spheres(case.sdf, case.resolution, case.xyzr, link, case.poses)


def test_nothing_to_compare_through_the_device_form(few_workgroups):
    """S == 0 and an empty grid: the kernel writes NO_VALUE (COLLISION under the flag for an empty grid), NaN and -1."""
    import torch
    case = C.case(6)
    b, links = case.poses.shape[:2]
    poses = torch.from_numpy(np.ascontiguousarray(case.poses)).cuda()
    xyzr = torch.from_numpy(np.ascontiguousarray(case.xyzr)).cuda()
    link = torch.from_numpy(np.ascontiguousarray(case.link)).cuda()
    sdf = torch.from_numpy(np.ascontiguousarray(case.sdf)).cuda()
    for s, shape, flag, status, outside in ((0, case.sdf.shape, True, 2, 0), (3, (12, 0, 9), False, 2, 3),
                                            (3, (0, 10, 9), True, 1, 3)):
        out = {"status": torch.full((b,), 77, dtype=torch.uint8, device="cuda"),
               "min_clearance": torch.zeros(b, dtype=torch.float64, device="cuda"),
               "min_sphere": torch.zeros(b, dtype=torch.int32, device="cuda"),
               "num_below": torch.full((b,), 5, dtype=torch.int32, device="cuda"),
               "num_outside": torch.full((b,), 5, dtype=torch.int32, device="cuda"),
               "min_gradient": torch.zeros((b, 3), dtype=torch.float64, device="cuda"),
               "sphere_clearance": torch.zeros((b, max(s, 1)), dtype=torch.float64, device="cuda")}
        torch.cuda.synchronize()
        few_workgroups.check_spheres_dev(sdf.data_ptr(), shape, case.resolution, xyzr.data_ptr(), link.data_ptr(), s,
                                         poses.data_ptr(), links, b, out["status"].data_ptr(),
                                         **{name + "_ptr": t.data_ptr() for name, t in out.items() if name != "status"},
                                         outside_is_collision=flag)
        few_workgroups.synchronize()
        got = {name: t.cpu().numpy() for name, t in out.items()}
        assert got["status"].tolist() == [status] * b and got["min_sphere"].tolist() == [-1] * b
        assert got["num_below"].tolist() == [0] * b and got["num_outside"].tolist() == [outside] * b
        assert np.isnan(got["min_clearance"]).all() and np.isnan(got["min_gradient"]).all()
        assert s == 0 or np.isnan(got["sphere_clearance"]).all()
