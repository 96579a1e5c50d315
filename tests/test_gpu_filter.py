"""(gpu) FilterKernel<float|double> and AccumulateCountsKernel at their edges, bit-equal to the numpy restatement of the
reference's rule (tests/filter_ref.py) and to the oracle library: ties and near-ties of the ratio in both precisions,
counts whose float conversion rounds, the outlier threshold, the camera rule, static occupancies around 0.5 and NaN, grids
with a tail and grids one launch cannot cover; the sum of a split cloud's shares on grids with a scalar tail and on one
beyond the launch cap.  tests/test_filter_ref.py shows on the CPU that these inputs discriminate."""
import numpy as np
import pytest

import filter_cases as C
import filter_ref as R
from conftest import bits_equal
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def narrow_ctx():
    c = capi.Context(0, C.SMALLEST_THREADS)
    yield c
    c.close()


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


def upload(ctx, case):
    """The case's counts in a new tracking-grid handle."""
    num_grids, cells, _ = case.tracking.shape
    grids = ctx.tracking_grids(cells, num_grids)
    ctx.synchronize()
    for g in range(num_grids):
        assert grids.offset(g) == g * cells * 2
        C.hip_memcpy_htod(grids.dev_ptr(g), case.tracking[g])
    return grids


def run_case(ctx, oracle, case):
    """Every option of the case in both precisions against the restatement and the oracle -> {(option, in_double): got}."""
    grids = upload(ctx, case)
    for g in range(case.tracking.shape[0]):
        assert np.array_equal(grids.retrieve(g), case.tracking[g])
    results = {}
    for option in case.options:
        percent, outlier, cameras = option
        for in_double in (False, True):
            fg = ctx.filter_grid(case.static)
            fg.filter(grids, percent, outlier, cameras, ratio_in_double=in_double)
            got = fg.retrieve()
            fg.close()
            assert bits_equal(got, R.filter_grids(case.tracking, case.static, percent, outlier, cameras, in_double)), \
                (case.name, option, in_double)
            assert bits_equal(got, oracle.filter_grids(case.tracking, case.static, percent, outlier, cameras, in_double)), \
                (case.name, option, in_double)
            results[option, in_double] = got
    grids.close()
    return results


def test_ties_and_near_ties(ctx, oracle):
    """The committed triples: the float and the double kernel differ on exactly the cells where the two rules do, in
    both directions."""
    (case,) = C.ties()
    results = run_case(ctx, oracle, case)
    float_free, float_filled = 0, 0
    for option in case.options:
        in_float, in_double = results[option, False], results[option, True]
        differ = R.filter_grids(case.tracking, case.static, *option, False) != \
            R.filter_grids(case.tracking, case.static, *option, True)
        assert np.array_equal(in_float != in_double, differ), option
        float_free += int(((in_float == 0.0) & (in_double == 1.0)).sum())
        float_filled += int(((in_float == 1.0) & (in_double == 0.0)).sum())
    assert float_free >= 8 and float_filled >= 8
    triples = C.tie_triples()
    for cell, (_, _, percent) in enumerate(triples):
        in_float, in_double = results[(percent, 1, 1), False][cell], results[(percent, 1, 1), True][cell]
        if cell < len(C.FLOAT_FREE_DOUBLE_FILLED):
            assert (in_float, in_double) == (0.0, 1.0), triples[cell]
        elif cell < len(C.FLOAT_FREE_DOUBLE_FILLED) + len(C.FLOAT_FILLED_DOUBLE_FREE):
            assert (in_float, in_double) == (1.0, 0.0), triples[cell]
        else:
            assert (in_float, in_double) == (0.0, 0.0), triples[cell]


def test_every_small_ratio_as_threshold(ctx, oracle):
    """percent_seen_free over every a / (a + b), 1 <= a, b <= 12, and the doubles either side: in double the ratio's own
    cells turn between the threshold and the double above it, in float all three are one threshold."""
    (case,) = C.ratio_sweep()
    results = run_case(ctx, oracle, case)
    pairs = case.tracking[0]
    for r in C.small_ratios():
        below, above = float(np.nextafter(r, 0.0)), float(np.nextafter(r, 1.0))
        own = [c for c, (a, b) in enumerate(pairs[:-2]) if a > 0 and b > 0 and a / (a + b) == r]
        assert own
        for p, want in ((below, 0.0), (r, 0.0), (above, 1.0)):
            assert (results[(p, 1, 1), True][own] == want).all(), (r, p)
        if np.float32(below) == np.float32(r) == np.float32(above):
            assert bits_equal(results[(below, 1, 1), False], results[(above, 1, 1), False])
            assert not bits_equal(results[(r, 1, 1), True], results[(above, 1, 1), True])


def test_counts_beyond_float_precision(ctx, oracle):
    (case,) = C.large_counts()
    assert set(np.unique(case.tracking).tolist()) == set(C.LARGE_COUNTS) | {0}
    results = run_case(ctx, oracle, case)
    assert any(not bits_equal(results[option, False], results[option, True]) for option in case.options)


def test_outlier_threshold(ctx, oracle):
    (case,) = C.outlier()
    results = run_case(ctx, oracle, case)
    for option in case.options:
        percent, t, cameras = option
        if cameras != 1:
            continue
        for in_double in (False, True):
            got = results[option, in_double]
            assert got[C.outlier_cell(0, t - 1)] == 0.5          # only evidence zeroed as an outlier: stays unknown
            assert got[C.outlier_cell(5, t - 1)] == 0.0          # with free > 0: seen free
            assert got[C.outlier_cell(0, t)] == 1.0 and got[C.outlier_cell(0, t + 1)] == 1.0


@pytest.mark.parametrize("index", range(len(C.CAMERA_GRIDS)), ids=["grids_%d" % g for g in C.CAMERA_GRIDS])
def test_camera_rule(ctx, oracle, index):
    case = C.camera()[index]
    grids = case.tracking.shape[0]
    results = run_case(ctx, oracle, case)
    for (percent, outlier, cameras), in_double in results:
        got = results[(percent, outlier, cameras), in_double]
        for k in range(grids + 1):
            assert got[C.camera_free_cell(grids, k, 0)] == (0.0 if k >= cameras else 0.5)
        for filled_camera in range(grids):
            assert got[C.camera_filled_cell(grids, filled_camera)] == 1.0


def test_static_occupancy_around_one_half(ctx, oracle):
    """Cells above 0.5 and NaN cells keep their bit pattern; everything at or below 0.5 is filtered."""
    (case,) = C.static()
    results = run_case(ctx, oracle, case)
    skipped = C.static_skipped()
    for got in results.values():
        assert bits_equal(got[skipped], case.static[skipped])
        assert np.isin(got[~skipped], (0.0, 0.5, 1.0)).all()
    assert any((got[~skipped] != case.static[~skipped]).any() for got in results.values())


@pytest.mark.parametrize("cells", C.SMALL_SIZES)
def test_grids_with_a_tail(ctx, narrow_ctx, oracle, cells):
    case = C.mixture(cells)
    run_case(ctx, oracle, case)
    run_case(narrow_ctx, oracle, case)


@pytest.mark.parametrize("threads", [C.DEFAULT_THREADS, C.SMALLEST_THREADS])
def test_grid_one_launch_cannot_cover(ctx, narrow_ctx, oracle, threads):
    """256 * 64 workgroups of the context's size, and 321 cells more: the kernel's loop comes round.  The last cell and
    the first cell past the cap are unknown cells that the filter changes."""
    context = ctx if threads == C.DEFAULT_THREADS else narrow_ctx
    cells = C.over_the_cap(threads)
    case = C.mixture(cells)
    marks = C.marked_cells(cells)
    assert marks[0] == cells - 1 and C.FILTER_MAX_WORKGROUPS * threads in marks
    assert not R.skipped(case.static)[marks].any()
    results = run_case(context, oracle, case)
    for got in results.values():
        assert (got[marks] != case.static[marks]).all()


def test_device_resident_filter(ctx, oracle):
    """Raycast -> filter -> the filtered grid's device buffer, nothing retrieved in between (the chain of
    test_device_resident_voxelize_then_sdf, stopped after the filter)."""
    from voxelized_geometry_tools_amd import synthetic
    counts = (33, 21, 19)
    vs = np.float32(0.05)
    ivs = np.float32(1.0) / vs
    sizes = [np.float32(c) * vs for c in counts]
    static = np.full(counts, 0.5, dtype=np.float32)
    static[:, :, 0] = 1.0
    static[5, 5, 5] = np.float32(np.nan)
    clouds = [synthetic.raycast_cloud(20_000, seed=7 + i) * np.float32(0.3) for i in range(2)]
    xfs = [synthetic.translation_xform(0.6 + 0.3 * i, 0.5, 0.4).astype(np.float32) for i in range(2)]
    grids = ctx.tracking_grids(int(np.prod(counts)), 2)
    fg = ctx.filter_grid(static)
    for i in range(2):
        grids.raycast_f32(i, clouds[i], 1.0, xfs[i], vs, ivs, sizes, counts)
    fg.filter(grids, 0.9, 2, 2)
    pointer = fg.dev_ptr()
    ctx.synchronize()
    got = C.hip_memcpy_dtoh(pointer, counts, np.float32)
    tracking = np.stack([oracle.raycast_f32(clouds[i], 1.0, xfs[i], vs, ivs, sizes, counts) for i in range(2)])
    want = R.filter_grids(tracking, static, 0.9, 2, 2, False)
    assert len(np.unique(want[~np.isnan(want)])) == 3
    assert bits_equal(got, want)
    assert bits_equal(got, oracle.filter_grids(tracking, static, 0.9, 2, 2, False))
    assert bits_equal(fg.retrieve(), want)
    fg.close()
    grids.close()


@pytest.mark.parametrize("counts,helpers", [(c, h) for c in C.SPLIT_GRIDS for h in C.SPLIT_HELPERS],
                         ids=["%dx%dx%d-%d_helpers" % (c + (len(h),)) for c in C.SPLIT_GRIDS for h in C.SPLIT_HELPERS])
def test_shares_summed_into_a_loaded_grid(ctx, counts, helpers):
    """vgt_hipx_raycast_points_split into grid 1 of a two-grid handle that already holds counts: they stay, every share's
    counts are added to the last int (the scalar tail where 2 * cells is no multiple of 4; the second round of the
    loop on the 162^3 grid), a second split adds again, and grid 0 is not touched."""
    scene = C.split_scene(counts)
    before, whole, again, _ = C.split_expected(counts)
    cells = int(np.prod(counts))
    grids = ctx.tracking_grids(cells, 2)
    ctx.synchronize()
    assert grids.offset(1) == 2 * cells
    C.hip_memcpy_htod(grids.dev_ptr(1), before)
    call = (scene.max_range, scene.xform, scene.voxel_size, scene.inverse_voxel_size, scene.sizes, scene.counts)
    grids.raycast_f32_split(1, helpers, scene.points, *call)
    assert np.array_equal(grids.retrieve(1, counts), before + whole)
    assert not grids.retrieve(0).any()
    grids.raycast_f32_split(1, helpers, scene.points[:100], *call)
    assert np.array_equal(grids.retrieve(1, counts), before + whole + again)
    assert not grids.retrieve(0).any()
    grids.close()
    capi.sdf_multi_release()
