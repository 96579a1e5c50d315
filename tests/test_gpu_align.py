"""(gpu) vgt_hip_align_points[_dev] against tests/align_ref.py, the CPU restatement of the call: every output bit-equal
(NaNs by position), through the host entry point of the product library and through the device entry point on torch
buffers -- the latter through the testing library with the evaluation limited to two workgroups, so that the shared
cases' (pose, 4096-point block) items make its persistent workgroups take several trips -- on the shapes of
tests/align_cases.py, which lie on either side of the item count at which the evaluation changes its workgroup size."""
import numpy as np
import pytest

import align_cases as C
import align_ref as R
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu

FIELDS = R.CloudAlignment._fields


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def few_workgroups():
    """A context of the testing library whose evaluation launches have at most two workgroups."""
    c = capi.Context(0, testing=True)
    c.set_align_workgroups(2)
    yield c
    c.set_align_workgroups(0)
    c.close()


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return np.array_equal(nan_a, nan_b) and np.array_equal(a[~nan_a].view(np.uint64), b[~nan_b].view(np.uint64))


def assert_same(got, want, what, leave_out=()):
    print(what, "statuses", np.bincount(got.status, minlength=4).tolist(), "evaluations",
          np.bincount(want.evaluations).tolist())
    for name in FIELDS:
        g, w = getattr(got, name), getattr(want, name)
        if name in leave_out:
            assert g is None, name
            continue
        assert g is not None and same_bits(g, w), (what, name)


def align_host(ctx, case):
    return ctx.align_points(case.sdf, case.resolution, case.points, case.poses, grid_from_world=case.grid_from_world,
                            rotation=case.rotation, **case.options)


def align_dev(ctx, case, leave_out=(), alias=False):
    """The device-pointer entry point on torch buffers; `leave_out`: outputs passed as NULL (returned as None);
    alias: poses_out is the input array."""
    import torch
    b, n = len(case.poses), len(case.points)
    sdf = torch.from_numpy(np.ascontiguousarray(case.sdf)).cuda()
    points = torch.from_numpy(np.ascontiguousarray(case.points)).cuda()
    poses = torch.from_numpy(np.ascontiguousarray(case.poses)).cuda()
    shapes = {"poses": ((b, 16), torch.float64), "status": ((b,), torch.uint8), "num_used": ((b,), torch.int32),
              "num_outside": ((b,), torch.int32), "num_rejected": ((b,), torch.int32),
              "sum_squared": ((b,), torch.float64), "evaluations": ((b,), torch.int32),
              "normal_equations": ((b, 27), torch.float64), "last_step": ((b, 6), torch.float64)}
    out = {name: torch.full(shape, 77, dtype=dtype, device="cuda") for name, (shape, dtype) in shapes.items()
           if name not in leave_out}
    if alias:
        out["poses"] = poses
    size = capi.align_points_workspace_bytes(n, b)
    assert size > 0
    workspace = torch.empty(size, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pointers = {("poses_out" if name == "poses" else name) + "_ptr": t.data_ptr() for name, t in out.items()}
    ctx.align_points_dev(sdf.data_ptr(), case.sdf.shape, case.resolution, points.data_ptr(), n, poses.data_ptr(), b,
                         workspace_ptr=workspace.data_ptr(), workspace_bytes=size, grid_from_world=case.grid_from_world,
                         rotation=case.rotation, **pointers, **case.options)
    ctx.synchronize()
    return R.CloudAlignment(*[out[name].cpu().numpy() if name in out else None for name in FIELDS])


@pytest.mark.parametrize("index", range(len(C.SHAPES)), ids=C.names())
def test_host_form(ctx, index):
    case = C.case(index)
    assert_same(align_host(ctx, case), case.want, case.name + " (host)")


@pytest.mark.parametrize("index", range(len(C.SHAPES)), ids=C.names())
def test_device_form_with_striding_workgroups(few_workgroups, index):
    case = C.case(index)
    assert_same(align_dev(few_workgroups, case), case.want, case.name + " (dev, 2 workgroups)")


def test_device_form_of_the_product_library(ctx):
    for index in (4, 9, 12):
        case = C.case(index)
        assert_same(align_dev(ctx, case), case.want, case.name + " (dev)")


def test_without_frame_and_pivot_and_with_four_by_four_poses(ctx):
    """The cases alternate the origin transform and leave the pivot out every third time; here neither is given, and the
    poses come as matrices."""
    case = C.case(5)
    assert case.grid_from_world is not None and case.options["pivot"] is None
    plain = C.case(8)
    assert plain.grid_from_world is None and plain.options["pivot"] is None
    matrices = case.poses.reshape(-1, 4, 4).transpose(0, 2, 1)
    got = ctx.align_points(case.sdf, case.resolution, case.points, matrices, grid_from_world=case.grid_from_world,
                           rotation=case.rotation, **case.options)
    assert_same(got, case.want, case.name + " (4 x 4)")


def test_optional_outputs_left_out_one_at_a_time(few_workgroups):
    case = C.case(4)                                                               # N257-B67-K1
    for name in FIELDS:
        if name == "status":
            continue
        assert_same(align_dev(few_workgroups, case, leave_out=(name,)), case.want, "without " + name, leave_out=(name,))
    everything = tuple(name for name in FIELDS if name != "status")
    assert_same(align_dev(few_workgroups, case, leave_out=everything), case.want, "status alone", leave_out=everything)


def test_poses_out_may_be_the_input(few_workgroups):
    for index in (7, 10):
        case = C.case(index)
        assert_same(align_dev(few_workgroups, case, alias=True), case.want, case.name + " (in place)")


def test_a_flat_wall_is_degenerate_on_the_device(ctx):
    sdf, res = C.wall(), C.RESOLUTION
    face = C.surface_centres(True)
    face = face[(face[:, 0] > 6 * res) & (np.abs(face[:, 1] - 14 * res) < 6 * res) & (np.abs(face[:, 2] - 18 * res) < 8 * res)]
    points = C.to_cloud(face + [0.3 * res, 0.0, 0.0])
    start = C.column_major(C.moved(C.truth(), 0.2, 0.0, 4))[None]
    options = dict(max_iterations=5, damping=1e-3, target_distance=-0.5 * res, pivot=C.centre())
    want = R.align(sdf, res, points, start, **options)
    assert want.status[0] == R.DEGENERATE
    assert_same(ctx.align_points(sdf, res, points, start, **options), want, "flat wall")


def test_three_levels_above_the_groups(ctx):
    """262 145 points: 65 blocks of 4096, so one launch of the level between the blocks and the solve."""
    n = 262145
    rng = np.random.default_rng(9)
    centres = C.surface_centres()
    world = centres[rng.integers(0, len(centres), n)] + (rng.random((n, 3)) - 0.5) * 0.8 * C.RESOLUTION
    points = C.to_cloud(world)
    start = C.column_major(C.moved(C.truth(), 0.5, 1.0, 2))[None]
    options = dict(max_iterations=0, target_distance=-0.5 * C.RESOLUTION, max_residual=1.5 * C.RESOLUTION,
                   pivot=C.centre())
    want = R.align(C.scene(), C.RESOLUTION, points, start, **options)
    assert want.status[0] == R.ITERATION_LIMIT and want.num_used[0] > 200000
    assert_same(ctx.align_points(C.scene(), C.RESOLUTION, points, start, **options), want, "N262145-B1-K0")
