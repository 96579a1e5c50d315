"""(gpu) vgt_hip_rasterize_spheres[_dev] and vgt_hip_spheres_cover_points[_dev] against tests/volume_ref.py, the CPU
restatement of the calls: every output bit-equal, through the host entry points of the product library and through the
device entry points on torch buffers -- the latter through the testing library with the launches limited to two
workgroups, so that the shared cases make the persistent waves and workgroups take several trips -- on the shapes of
tests/volume_cases.py; and two checks of the device's outputs against each other."""
import numpy as np
import pytest

import volume_cases as C
import volume_ref as R
from voxelized_geometry_tools_amd import capi, synthetic

pytestmark = pytest.mark.gpu

GRID_INDICES = range(len(C.SHAPES))
POINT_NUMBERS = range(len(C.POINT_CASES))
OUTPUTS = R.PointCover._fields


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def few_workgroups():
    """A context of the testing library whose sphere-volume launches have at most two workgroups (eight waves, 512 points)."""
    c = capi.Context(0, testing=True)
    c.set_sphere_volume_workgroups(2)
    yield c
    c.set_sphere_volume_workgroups(0)
    c.close()


@pytest.fixture(scope="module", autouse=True)
def conditions():
    print(C.check_conditions())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return np.array_equal(nan_a, nan_b) and np.array_equal(a[~nan_a].view(np.uint32), b[~nan_b].view(np.uint32))


def model_on_device(xyzr, link, poses):
    import torch
    # (copies: the shared cases are read-only)
    return (torch.from_numpy(np.array(xyzr, dtype=np.float64)).cuda(), torch.from_numpy(np.array(link, dtype=np.int32)).cuda(),
            torch.from_numpy(np.array(poses, dtype=np.float64)).cuda())


def rasterize_dev(ctx, case, shape=None, xyzr=None, link=None, poses=None, base=0, into=None):
    """The device-pointer entry point on torch buffers; into: the int32 array to keep and lower."""
    import torch
    shape = case.shape if shape is None else shape
    xyzr = case.xyzr if xyzr is None else xyzr
    link = case.link if link is None else link
    poses = case.poses if poses is None else poses
    d_xyzr, d_link, d_poses = model_on_device(xyzr, link, poses)
    if into is None:
        first = torch.full(tuple(shape), 77, dtype=torch.int32, device="cuda")
    else:
        first = torch.from_numpy(np.array(into, dtype=np.int32)).cuda()
    anchor = torch.zeros(1, dtype=torch.int32, device="cuda")                       # (an empty tensor has no address)
    torch.cuda.synchronize()
    ctx.rasterize_spheres_dev(shape, case.resolution, d_xyzr.data_ptr(), d_link.data_ptr(), len(xyzr), d_poses.data_ptr(),
                              poses.shape[1], poses.shape[0], first.data_ptr() or anchor.data_ptr(), padding=case.padding,
                              base=base,
                              keep=into is not None, grid_from_world=case.grid_from_world)
    ctx.synchronize()
    return first.cpu().numpy()


def cover_dev(ctx, case, leave_out=(), alias=False, link=None, points=None):
    """-> PointCover with None for the outputs in `leave_out`; alias: filtered_xyz is the input array itself."""
    import torch
    link = case.link if link is None else link
    points = case.points if points is None else points
    n = len(points)
    d_xyzr, d_link, d_poses = model_on_device(case.xyzr, link, case.poses)
    d_points = torch.from_numpy(np.array(points, dtype=np.float32)).cuda()
    out = {"first_configuration": torch.full((n,), 77, dtype=torch.int32, device="cuda"),
           "first_sphere": torch.full((n,), 77, dtype=torch.int32, device="cuda"),
           "filtered": d_points if alias else torch.full((n, 3), 77.0, dtype=torch.float32, device="cuda")}
    out = {name: t for name, t in out.items() if name not in leave_out}
    torch.cuda.synchronize()
    ctx.spheres_cover_points_dev(d_points.data_ptr(), n, d_xyzr.data_ptr(), d_link.data_ptr(), len(case.xyzr),
                                 d_poses.data_ptr(), case.poses.shape[1], case.poses.shape[0],
                                 **{name + "_ptr": t.data_ptr() for name, t in out.items()}, padding=case.padding,
                                 world_from_points=case.world_from_points)
    ctx.synchronize()
    if not alias:
        assert same_bits(d_points.cpu().numpy(), points)                            # the input is read-only
    return R.PointCover(*[out[name].cpu().numpy() if name in out else None for name in OUTPUTS])


def assert_cover(got, want, what, leave_out=()):
    found = got.first_configuration if got.first_configuration is not None else want.first_configuration
    print(what, "covered", int((found >= 0).sum()), "of", len(found))
    for name in OUTPUTS:
        g, w = getattr(got, name), getattr(want, name)
        if name in leave_out:
            assert g is None, name
        else:
            assert g is not None and same_bits(g, w), (what, name)


def assert_grid(got, want, what):
    print(what, "covered", int((got >= 0).sum()), "of", got.size, "configurations", len(np.unique(got[got >= 0])))
    assert got.dtype == np.int32 and got.shape == want.shape and np.array_equal(got, want), what


@pytest.mark.parametrize("index", GRID_INDICES, ids=C.names())
def test_grid_host_form(ctx, index):
    case = C.case(index)
    got = ctx.rasterize_spheres(case.shape, case.resolution, case.xyzr, case.link, case.poses, case.padding,
                                grid_from_world=case.grid_from_world)
    assert_grid(got, case.want, case.name + " (host)")


@pytest.mark.parametrize("index", GRID_INDICES, ids=C.names())
def test_grid_device_form_with_striding_waves(few_workgroups, index):
    case = C.case(index)
    assert_grid(rasterize_dev(few_workgroups, case), case.want, case.name + " (dev, 2 workgroups)")


def test_grid_device_form_of_the_product_library(ctx):
    for index in (4, 15, 21):
        case = C.case(index)
        assert_grid(rasterize_dev(ctx, case), case.want, case.name + " (dev)")


@pytest.mark.parametrize("number", POINT_NUMBERS, ids=C.point_names())
def test_point_host_form(ctx, number):
    case = C.point_case(number)
    got = ctx.spheres_cover_points(case.points, case.xyzr, case.link, case.poses, case.padding, case.world_from_points,
                                   filtered=True)
    assert_cover(got, case.want, case.name + " (host)")
    brief = ctx.spheres_cover_points(case.points, case.xyzr, case.link, case.poses, case.padding, case.world_from_points)
    assert_cover(brief, case.want, case.name + " (host, no filtered)", leave_out=("filtered",))


@pytest.mark.parametrize("number", POINT_NUMBERS, ids=C.point_names())
def test_point_device_form_with_striding_workgroups(few_workgroups, number):
    case = C.point_case(number)
    assert_cover(cover_dev(few_workgroups, case), case.want, case.name + " (dev, 2 workgroups)")


def test_point_device_form_of_the_product_library(ctx):
    for number in (4, 5, 11):
        case = C.point_case(number)
        assert_cover(cover_dev(ctx, case), case.want, case.name + " (dev)")


@pytest.mark.parametrize("number", [3, 11], ids=[C.point_names()[3], C.point_names()[11]])
def test_point_outputs_left_out_one_at_a_time(few_workgroups, number):
    case = C.point_case(number)
    for name in OUTPUTS:
        assert_cover(cover_dev(few_workgroups, case, leave_out=(name,)), case.want, case.name + " without " + name,
                     leave_out=(name,))
        only = tuple(other for other in OUTPUTS if other != name)
        assert_cover(cover_dev(few_workgroups, case, leave_out=only), case.want, case.name + " only " + name,
                     leave_out=only)


@pytest.mark.parametrize("number", [4, 5], ids=[C.point_names()[4], C.point_names()[5]])
def test_filtered_may_be_the_input_array(few_workgroups, number):
    case = C.point_case(number)
    assert_cover(cover_dev(few_workgroups, case, alias=True), case.want, case.name + " (in place)")
    assert_cover(cover_dev(few_workgroups, case, alias=True, leave_out=OUTPUTS[:2]), case.want,
                 case.name + " (in place, alone)", leave_out=OUTPUTS[:2])


@pytest.mark.parametrize("index", [6, 10, 20], ids=[C.names()[i] for i in (6, 10, 20)])
def test_keep_merges_two_calls_with_rising_bases_in_either_order(few_workgroups, ctx, index):
    case = C.case(index)
    cut = case.poses.shape[0] // 3
    low, high = case.poses[:cut], case.poses[cut:]
    want = case.want.copy()
    want[want >= 0] += 1000
    whole = rasterize_dev(few_workgroups, case, base=1000)
    assert_grid(whole, want, case.name + " (base 1000)")
    first = rasterize_dev(few_workgroups, case, poses=low, base=1000)
    assert_grid(rasterize_dev(few_workgroups, case, poses=high, base=1000 + cut, into=first), want, "low, then high")
    first = rasterize_dev(few_workgroups, case, poses=high, base=1000 + cut)
    assert (first[first >= 0] >= 1000 + cut).all()
    assert_grid(rasterize_dev(few_workgroups, case, poses=low, base=1000, into=first), want, "high, then low")
    # the host form uploads the array it keeps
    first = ctx.rasterize_spheres(case.shape, case.resolution, case.xyzr, case.link, high, case.padding, base=1000 + cut,
                                  grid_from_world=case.grid_from_world)
    kept = ctx.rasterize_spheres(case.shape, case.resolution, case.xyzr, case.link, low, case.padding, base=1000,
                                 into=first, grid_from_world=case.grid_from_world)
    assert kept is first
    assert_grid(first, want, "high, then low (host)")


def test_a_link_out_of_range_through_the_device_forms_covers_nothing(few_workgroups):
    case = C.case(12)                                                               # S = 33 + 2, L = 3
    link = case.link.copy()
    link[[0, 7, 32]] = [3, -1, 2 ** 31 - 1]
    want = R.rasterize_spheres(case.shape, case.resolution, case.xyzr, link, case.poses, case.padding, 0, None,
                               case.grid_from_world)
    assert not np.array_equal(want, case.want) and (want >= 0).any()
    assert_grid(rasterize_dev(few_workgroups, case, link=link), want, case.name + " (links out of range)")
    with pytest.raises(ValueError, match="sphere 0: link 3"):
        few_workgroups.rasterize_spheres(case.shape, case.resolution, case.xyzr, link, case.poses)
    points = C.point_case(3)                                                        # over the same model
    assert points.xyzr is case.xyzr
    want = R.spheres_cover_points(points.points, points.xyzr, link, points.poses, points.padding,
                                  points.world_from_points)
    assert (want.first_configuration >= 0).any()
    assert_cover(cover_dev(few_workgroups, points, link=link), want, points.name + " (links out of range)")
    with pytest.raises(ValueError, match="sphere 0: link 3"):
        few_workgroups.spheres_cover_points(points.points, points.xyzr, link, points.poses)


def test_nothing_to_cover_with_through_the_device_forms(few_workgroups):
    """S == 0, B == 0 and an empty grid: -1 everywhere unless kept; -1 and the plain copy for the points."""
    case = C.case(6)
    points = C.point_case(4)
    no_spheres = dict(xyzr=case.xyzr[:0], link=case.link[:0])
    no_poses = dict(poses=case.poses[:0])
    for kw in (no_spheres, no_poses):
        assert (rasterize_dev(few_workgroups, case, **kw) == -1).all()
        kept = np.arange(np.prod(case.shape), dtype=np.int32).reshape(case.shape) - 5
        assert np.array_equal(rasterize_dev(few_workgroups, case, into=kept, **kw), kept)
    assert rasterize_dev(few_workgroups, case, shape=(24, 0, 19)).shape == (24, 0, 19)
    plain = R.PointCover(np.full(len(points.points), -1, np.int32), np.full(len(points.points), -1, np.int32),
                         points.points)
    assert_cover(cover_dev(few_workgroups, points._replace(poses=points.poses[:0])), plain, "B == 0")
    assert_cover(cover_dev(few_workgroups, points._replace(xyzr=points.xyzr[:0]), link=points.link[:0]), plain, "S == 0")
    none = few_workgroups.spheres_cover_points(points.points[:0], points.xyzr, points.link, points.poses, filtered=True)
    assert [len(a) for a in none] == [0, 0, 0]


@pytest.mark.parametrize("index", [6, 13], ids=[C.names()[i] for i in (6, 13)])
def test_the_counting_kernel_counts_what_the_restatement_covers(few_workgroups, index):
    """The testing library's counting run (what tools/bench_volumes.py takes its atomic share from): the same answer, the
    covering tests of the brute-force restatement exactly, at least one atomic per covered cell and at most one per
    covering test, and no fewer tests than covering ones."""
    import torch
    case = C.case(index)
    c, radius, usable = R.usable_spheres(case.xyzr, case.link, case.poses, case.padding, case.grid_from_world)
    axes = R.cell_centre_axes(case.shape, case.resolution)
    covering = sum(int(R._covers_cells(axes, c[b, s], radius[s]).sum()) for b, s in np.argwhere(usable))
    counters = torch.zeros(3, dtype=torch.int64, device="cuda")
    few_workgroups.set_sphere_volume_counters(counters.data_ptr())
    try:
        got = rasterize_dev(few_workgroups, case)
    finally:
        few_workgroups.set_sphere_volume_counters(None)
    tests, counted, atomics = counters.cpu().numpy().tolist()
    print(case.name, "tests", tests, "covering", counted, "atomics", atomics, "covered cells", int((got >= 0).sum()))
    assert_grid(got, case.want, case.name + " (counting)")
    assert counted == covering > 0 and tests >= counted
    assert int((got >= 0).sum()) <= atomics <= counted
    assert_grid(rasterize_dev(few_workgroups, case), case.want, case.name + " (after counting)")
    assert counters.cpu().numpy().tolist() == [tests, counted, atomics]              # (the hook is off again)


@pytest.mark.parametrize("index", [4, 10, 18], ids=[C.names()[i] for i in (4, 10, 18)])
def test_the_point_form_on_cell_centres_is_the_grid_form(ctx, index):
    """On the device's own outputs, without the restatement: the float32 cell centres are exact at this resolution."""
    case = C.case(index)
    assert case.grid_from_world is None
    first = ctx.rasterize_spheres(case.shape, case.resolution, case.xyzr, case.link, case.poses, case.padding)
    centres = R.cell_centres(case.shape, case.resolution).reshape(-1, 3)
    points = centres.astype(np.float32)
    assert np.array_equal(points.astype(np.float64), centres)
    got = ctx.spheres_cover_points(points, case.xyzr, case.link, case.poses, case.padding)
    print(case.name, "covered", int((first >= 0).sum()), "of", first.size)
    assert (first >= 0).any() and np.array_equal(got.first_configuration, first.reshape(-1))
    assert np.array_equal(got.first_sphere >= 0, got.first_configuration >= 0)


def test_a_self_filtered_cloud_raycasts_like_the_cloud_without_the_covered_points(ctx):
    """The composition the feature exists for: spheres_cover_points(filtered=True) -> raycast_f32 against the same cloud
    with the covered points removed by numpy.  The raycast skips non-finite points, so the tracking counts are
    identical."""
    counts = (32, 32, 32)
    vs = np.float32(0.05)
    cloud = synthetic.raycast_cloud(6000, seed=5) * np.float32(0.4)
    xf = synthetic.translation_xform(0.8, 0.8, 0.8).astype(np.float32)
    sizes = [np.float32(c) * vs for c in counts]
    # a "robot" in the cloud's frame: spheres around some of the cloud's own points, one configuration, two links
    rng = np.random.default_rng(9)
    on_robot = cloud[rng.choice(len(cloud), 12, replace=False)].astype(np.float64)
    xyzr = np.concatenate([on_robot - [0.1, 0.0, 0.0], np.full((12, 1), 0.08)], axis=1)
    link = (np.arange(12) % 2).astype(np.int32)
    poses = np.tile(np.eye(4).reshape(16), (1, 2, 1))
    poses[0, :, 12] = 0.1
    cover = ctx.spheres_cover_points(cloud, xyzr, link, poses, filtered=True)
    covered = cover.first_configuration >= 0
    print("covered", int(covered.sum()), "of", len(cloud))
    assert 12 <= covered.sum() < len(cloud) // 2
    assert np.isnan(cover.filtered[covered]).all() and same_bits(cover.filtered[~covered], cloud[~covered])

    def tracking(points):
        grids = ctx.tracking_grids(int(np.prod(counts)), 1)
        grids.raycast_f32(0, points, 1.0, xf, vs, np.float32(1.0) / vs, sizes, counts)
        got = grids.retrieve(0, counts)
        grids.close()
        return got

    filtered, removed, unfiltered = tracking(cover.filtered), tracking(cloud[~covered]), tracking(cloud)
    assert np.array_equal(filtered, removed)
    assert not np.array_equal(filtered, unfiltered)                                  # (the filter took something away)
