"""(gpu) vgt_hip_sdf_project_out_of_collision[_dev] against tests/projection_ref.py, the CPU restatement of
ProjectLocationOutOfCollisionToMinimumDistance: status, has_value and iterations equal, positions bit-identical (NaN
patterns included), on the smallest scenes at which each branch can go wrong (tests/projection_cases.py)."""
import math

import numpy as np
import pytest

import projection_cases as C
import projection_ref as P
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


def same_doubles(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(nan_a, nan_b) and \
        np.array_equal(a[~nan_a].view(np.uint64), b[~nan_b].view(np.uint64))


def assert_same(got, want, what):
    pos, has, status, iterations = got
    wpos, whas, wstatus, witerations = want
    counts = np.bincount(status, minlength=5).tolist()
    print(what, "statuses", counts, "most steps", int(iterations.max(initial=0)))
    assert status.dtype == np.uint8 and iterations.dtype == np.int32 and pos.shape == wpos.shape
    assert np.array_equal(status, wstatus), (what, counts, np.bincount(wstatus, minlength=5).tolist())
    assert np.array_equal(has, whas), what
    assert np.array_equal(iterations, witerations), what
    assert same_doubles(pos, wpos), what


def project_dev(ctx, occupancy, res, queries, **kw):
    """The device-pointer entry point straight after vgt_hip_sdf_dev: the field never visits the host."""
    import torch
    shape = occupancy.shape
    occ = torch.from_numpy(np.ascontiguousarray(occupancy, dtype=np.float32)).cuda()
    sdf = torch.empty(shape, dtype=torch.float32, device="cuda")
    nbytes = capi.sdf_workspace_bytes(shape)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    q = torch.from_numpy(np.ascontiguousarray(queries, dtype=np.float64)).cuda()
    n = len(queries)
    pos = torch.empty((n, 3), dtype=torch.float64, device="cuda")
    has = torch.empty(n, dtype=torch.uint8, device="cuda")
    status = torch.empty(n, dtype=torch.uint8, device="cuda")
    iterations = torch.empty(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ctx.sdf_dev(occ.data_ptr(), shape, res, sdf.data_ptr(), ws.data_ptr(), nbytes)
    ctx.sdf_project_out_of_collision_dev(sdf.data_ptr(), shape, res, q.data_ptr(), n, pos.data_ptr(), has.data_ptr(),
                                         status.data_ptr(), iterations.data_ptr(), **kw)
    ctx.synchronize()
    return pos.cpu().numpy(), has.cpu().numpy().astype(bool), status.cpu().numpy(), iterations.cpu().numpy()


CASES = [("spheres", 0.0, 0), ("spheres", 1.5, 0), ("dense", 0.0, 0), ("corridor", 3.0, 0), ("corridor", 3.0, 7),
         ("corridor", 0.0, 0), ("flat_1x6x5", 0.0, 0), ("tiny_2x2x2", 0.0, 0), ("one_voxel", 0.0, 0)]


@pytest.mark.parametrize("name,clearance_cells,max_iterations", CASES)
def test_projection_matches_the_restatement(ctx, oracle, name, clearance_cells, max_iterations):
    sdf, res = C.scene(name)
    occ, _ = C.occupancy(name)
    q = C.queries(name)
    minimum_distance = clearance_cells * res
    want = P.project_out_of_collision(oracle, sdf, res, q, minimum_distance, 0.1, max_iterations)
    got = ctx.sdf_project_out_of_collision(sdf, res, q, minimum_distance, 0.1, max_iterations)
    assert_same(got, want, (name, clearance_cells, max_iterations, "host"))
    got = project_dev(ctx, occ, res, q, minimum_distance=minimum_distance, max_iterations=max_iterations)
    assert_same(got, want, (name, clearance_cells, max_iterations, "dev"))
    if name == "corridor" and clearance_cells > 0:
        assert (got[2] == capi.PROJECT_ITERATION_LIMIT).all() and (got[3] == (max_iterations or 520)).all()
    if name == "corridor" and clearance_cells == 0:
        assert (got[2] == capi.PROJECT_OK).all() and got[3].max() <= 15


def test_frames_and_step_size(ctx, oracle):
    """A grid_from_world / rotation pair (rotation about z plus a translation) and a second step size, through both
    entry points."""
    sdf, res = C.scene("spheres")
    occ, _ = C.occupancy("spheres")
    grid_from_world, rotation, world_from_grid = C.frame_pair()
    q = C.to_world(C.queries("spheres"), world_from_grid)
    want = P.project_out_of_collision(oracle, sdf, res, q, 0.0, 0.1, 0, grid_from_world, rotation)
    assert len(np.unique(want[2])) >= 3
    got = ctx.sdf_project_out_of_collision(sdf, res, q, grid_from_world=grid_from_world, rotation=rotation)
    assert_same(got, want, "frames host")
    got = project_dev(ctx, occ, res, q, grid_from_world=grid_from_world, rotation=rotation)
    assert_same(got, want, "frames dev")
    want = P.project_out_of_collision(oracle, sdf, res, q, 0.5 * res, 0.37, 0, grid_from_world, rotation)
    got = ctx.sdf_project_out_of_collision(sdf, res, q, 0.5 * res, 0.37, 0, grid_from_world, rotation)
    assert_same(got, want, "frames, multiplier 0.37")


def test_default_iteration_limit(ctx):
    """max_iterations = 0 is ceil(2 * (nx + ny + nz) / stepsize_multiplier), passed explicitly."""
    for name, clearance_cells, multiplier in (("spheres", 1.5, 0.1), ("corridor", 3.0, 0.1), ("corridor", 3.0, 0.3)):
        sdf, res = C.scene(name)
        q = C.queries(name)
        limit = int(math.ceil(2 * sum(sdf.shape) / multiplier))
        default = ctx.sdf_project_out_of_collision(sdf, res, q, clearance_cells * res, multiplier, 0)
        explicit = ctx.sdf_project_out_of_collision(sdf, res, q, clearance_cells * res, multiplier, limit)
        assert_same(default, explicit, (name, "default limit"))
        at_limit = default[2] == capi.PROJECT_ITERATION_LIMIT
        assert at_limit.any() and (default[3][at_limit] == limit).all()
        one_less = ctx.sdf_project_out_of_collision(sdf, res, q, clearance_cells * res, multiplier, limit - 1)
        assert (one_less[3][one_less[2] == capi.PROJECT_ITERATION_LIMIT] == limit - 1).all()


def test_optional_outputs(ctx):
    """has_value, status and iterations may each be NULL without a change to the others."""
    sdf, res = C.scene("dense")
    q = np.ascontiguousarray(C.queries("dense"))
    full = ctx.sdf_project_out_of_collision(sdf, res, q)
    field = np.ascontiguousarray(sdf)
    for drop in ((0,), (1,), (2,), (0, 1, 2)):
        pos = np.empty((len(q), 3))
        outs = [np.full(len(q), 0xAB, np.uint8), np.full(len(q), 0xAB, np.uint8), np.full(len(q), -7, np.int32)]
        ptrs = [None if k in drop else capi._ptr(a) for k, a in enumerate(outs)]
        capi.check(ctx._lib.vgt_hip_sdf_project_out_of_collision(
            ctx.handle, capi._ptr(field), *field.shape, res, None, None, capi._ptr(q), len(q), 0.0, 0.1, 0,
            capi._ptr(pos), *ptrs))
        assert same_doubles(pos, full[0])
        for k, (out, want) in enumerate(zip(outs, (full[1].astype(np.uint8), full[2], full[3]))):
            if k in drop:
                assert (out == (0xAB if k < 2 else -7)).all()
            else:
                assert np.array_equal(out, want)
    assert ctx.sdf_project_out_of_collision(sdf, res, np.empty((0, 3)))[0].shape == (0, 3)


def test_argument_errors(ctx):
    sdf, res = C.scene("one_voxel")
    q = np.array([[0.25, 0.25, 0.25]])
    for kw in ({"stepsize_multiplier": 0.0}, {"stepsize_multiplier": -0.1}, {"stepsize_multiplier": math.nan},
               {"stepsize_multiplier": math.inf}, {"minimum_distance": math.nan}, {"max_iterations": -1}):
        with pytest.raises(ValueError):
            ctx.sdf_project_out_of_collision(sdf, res, q, **kw)
    for bad in (0.0, -0.1, math.nan):
        with pytest.raises(ValueError):
            ctx.sdf_project_out_of_collision(sdf, bad, q)
    # infinite clearances are values like any other: nothing clears +inf, everything in the grid clears -inf
    got = ctx.sdf_project_out_of_collision(sdf, res, q, math.inf, max_iterations=3)
    assert got[2].tolist() == [capi.PROJECT_FLAT_GRADIENT]
    got = ctx.sdf_project_out_of_collision(sdf, res, q, -math.inf)
    assert got[2].tolist() == [capi.PROJECT_OK] and same_doubles(got[0], q)


def test_every_status_occurs_on_the_device(ctx):
    """A comparison that never leaves OK shows nothing: the cases above are there for all five outcomes."""
    everything = {capi.PROJECT_OK, capi.PROJECT_OUTSIDE, capi.PROJECT_FLAT_GRADIENT, capi.PROJECT_LEFT_GRID,
                  capi.PROJECT_ITERATION_LIMIT}
    sdf, res = C.scene("spheres")
    _, _, status, _ = ctx.sdf_project_out_of_collision(sdf, res, C.queries("spheres"), 1.5 * res)
    assert set(int(s) for s in np.unique(status)) == everything
    seen = set()
    for name in ("spheres", "dense", "flat_1x6x5"):
        sdf, res = C.scene(name)
        seen.update(int(s) for s in np.unique(ctx.sdf_project_out_of_collision(sdf, res, C.queries(name))[2]))
    assert seen == everything, seen
