"""(gpu) Connected components, spatial segments and component surfaces on the device against the CPU yardsticks of
tests/components_ref.py.  Every comparison is np.array_equal on the whole uint32 label grid plus the count."""
import numpy as np
import pytest

import components_ref as R
from conftest import tagged_records
from voxelized_geometry_tools_amd import capi, synthetic

pytestmark = pytest.mark.gpu

# (record dtype or None = a plain float grid, object id offset): the four cell layouts of 4, 8, 8 and 16 bytes
LAYOUTS = [(None, -1), (capi.OCCUPANCY_COMPONENT_CELL, -1), (capi.TAGGED_OBJECT_CELL, 4),
           (capi.TAGGED_OBJECT_COMPONENT_CELL, 4)]
LAYOUT_IDS = ["float4", "component8", "tagged8", "tagged16"]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _records(occ, ids, dtype):
    if dtype is None:
        return np.ascontiguousarray(occ, dtype=np.float32)
    rec = np.zeros(occ.shape, dtype=dtype)
    rec["occupancy"] = occ
    if "object_id" in dtype.names:
        rec["object_id"] = ids
    if "component" in dtype.names:
        rec["component"] = 0xABCD0123          # what the cells hold before must not matter
    if "spatial_segment" in dtype.names:
        rec["spatial_segment"] = 0xDEADBEEF
    return rec


def _same(got, want):
    return got[0].dtype == np.uint32 and got[0].shape == want[0].shape and np.array_equal(got[0], want[0]) and \
        got[1] == want[1]


def _small_cases():
    cases = [(occ, np.zeros(occ.shape, np.uint32)) for _, occ, _, _ in R.hand_cases()]
    return cases + R.random_small_grids(200)


def test_hand_derived_labels(ctx):
    for name, occ, want, count in R.hand_cases():
        got = ctx.connected_components(occ)
        assert _same(got, (want, count)), name


def test_small_grids_plain_entry_point(ctx):
    cases = _small_cases()
    assert len(cases) >= 206
    for occ, _ in cases:
        assert _same(ctx.connected_components(occ), R.occupancy_labels_flood(occ)), occ.shape


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_IDS)
def test_small_grids_through_cells(ctx, layout):
    dtype, offset = layout
    for occ, ids in _small_cases():
        cells = ctx.cells(_records(occ, ids, dtype), occ.shape, object_id_offset=offset)
        across = R.occupancy_labels_flood(occ)
        assert _same(cells.connected_components(connect_across_objects=True), across), occ.shape
        by_object = R.occupancy_labels_flood(occ, ids) if offset >= 0 else across   # (no ids: the flag is ignored)
        assert _same(cells.connected_components(connect_across_objects=False), by_object), occ.shape
        cells.close()


def _snake(shape):
    """Filled walls with one empty corridor that runs along every second Z line and turns at alternating ends: a single
    component whose smallest index is far from most of its cells."""
    nx, ny, nz = shape
    occ = np.ones(shape, np.float32)
    lines = []
    for k, x in enumerate(range(0, nx, 2)):
        ys = list(range(0, ny, 2))
        lines += [(x, y) for y in (ys if k % 2 == 0 else ys[::-1])]
    for k, (x, y) in enumerate(lines):
        occ[x, y, :] = 0.0
        if k + 1 < len(lines):
            x2, y2 = lines[k + 1]
            occ[(x + x2) // 2, (y + y2) // 2, nz - 1 if k % 2 == 0 else 0] = 0.0
    return occ


def _stage_cases():
    rng = np.random.default_rng(5)
    cases = []
    for shape in ((1, 1, 1), (1, 1, 70), (1, 70, 1), (70, 1, 1), (3, 5, 257), (65, 63, 130)):
        # long runs with a few breaks, so that runs cross wave boundaries
        occ = (rng.random(shape) < 0.03).astype(np.float32)
        occ[rng.random(shape) < 0.01] = 0.5
        cases.append(("runs%s" % (shape,), occ))
        cases.append(("noise%s" % (shape,), rng.choice(R.OCCUPANCY_VALUES, size=shape).astype(np.float32)))
    cases.append(("snake", _snake((17, 15, 130))))
    x, y, z = np.meshgrid(np.arange(40), np.arange(33), np.arange(65), indexing="ij")
    cases.append(("checkerboard", ((x + y + z) % 2).astype(np.float32)))
    cases.append(("all_equal", np.full((33, 40, 129), 0.5, np.float32)))
    return cases


def test_shapes_that_stress_each_stage(ctx):
    for name, occ in _stage_cases():
        want = R.occupancy_labels_flood(occ) if occ.size <= 48 ** 3 else R.occupancy_labels_fast(occ)
        got = ctx.connected_components(occ)
        assert _same(got, want), name
        if name == "snake":
            corridor = occ == 0.0
            assert len(np.unique(got[0][corridor])) == 1 and got[0][0, 0, 0] == 1
        if name == "checkerboard":
            assert got[1] == occ.size and np.array_equal(got[0].reshape(-1), np.arange(1, occ.size + 1))
        if name == "all_equal":
            assert got[1] == 1 and (got[0] == 1).all()


def _flood_equals_fast_on(cases):
    for name, occ in cases:
        if occ.size <= 48 ** 3:
            assert _same(R.occupancy_labels_fast(occ), R.occupancy_labels_flood(occ)), name


def test_the_fast_yardstick_on_the_stage_cases():
    """The stage cases above that are too large for the flood fill use fast_labels; show it on the ones that are not."""
    _flood_equals_fast_on(_stage_cases())


LARGE = (256, 256, 256)


@pytest.fixture(scope="module")
def large_cases():
    out = {}
    for dist in ("spheres", "salt", "unknown_mix"):
        occ = synthetic.make_occupancy(LARGE, dist, seed=42)
        out[dist] = (occ, R.occupancy_labels_fast(occ))
    return out


@pytest.mark.parametrize("dist", ["spheres", "salt", "unknown_mix"])
def test_synthetic_256_host_and_device_pointers(ctx, large_cases, dist):
    import torch
    occ, want = large_cases[dist]
    assert _same(ctx.connected_components(occ), want)
    occ_dev = torch.from_numpy(occ).cuda()
    labels_dev = torch.zeros(LARGE, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    count = ctx.connected_components_dev(occ_dev.data_ptr(), LARGE, labels_dev.data_ptr())
    assert _same((labels_dev.cpu().numpy().view(np.uint32), count), want)


def test_chained_after_the_voxelizer_filter_on_the_device(ctx):
    """raycast -> filter -> labels without leaving the device: the filtered grid's device buffer is the input."""
    import torch
    counts = (96, 80, 64)
    vs = np.float32(0.05)
    ivs = np.float32(1.0) / vs
    sizes = [np.float32(c) * vs for c in counts]
    static = np.full(counts, 0.5, np.float32)
    grids = ctx.tracking_grids(int(np.prod(counts)), 2)
    for i in range(2):
        cloud = synthetic.raycast_cloud(40_000, seed=7 + i) * np.float32(0.6)
        xf = synthetic.translation_xform(2.0 + i, 2.0, 1.6).astype(np.float32)
        grids.raycast_f32(i, cloud, 4.0, xf, vs, ivs, sizes, counts)
    fg = ctx.filter_grid(static)
    fg.filter(grids, 0.9, 1, 1)
    labels_dev = torch.zeros(counts, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    count = ctx.connected_components_dev(fg.dev_ptr(), counts, labels_dev.data_ptr())
    occ = fg.retrieve()
    assert len(np.unique(occ)) == 3
    assert _same((labels_dev.cpu().numpy().view(np.uint32), count), R.occupancy_labels_fast(occ))
    fg.close()
    grids.close()


def test_labelling_is_deterministic(ctx, large_cases):
    import torch
    occ, want = large_cases["salt"]
    occ_dev = torch.from_numpy(occ).cuda()
    for _ in range(5):
        labels_dev = torch.zeros(LARGE, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        count = ctx.connected_components_dev(occ_dev.data_ptr(), LARGE, labels_dev.data_ptr())
        assert _same((labels_dev.cpu().numpy().view(np.uint32), count), want)


# ---- spatial segments ----
FACTORS = (0.5, 1.75, 3.3, 1.0e6)     # thresholds in units of the resolution; the last connects everything


@pytest.mark.parametrize("dtype", [capi.TAGGED_OBJECT_CELL, capi.TAGGED_OBJECT_COMPONENT_CELL], ids=["tagged8", "tagged16"])
def test_spatial_segments_on_synthetic_extrema_small(ctx, dtype):
    res = 0.25
    for k, (occ, ids) in enumerate(R.random_small_grids(60, seed=4242)):
        extrema = R.lattice_extrema(occ.shape, res, seed=9000 + k)
        cells = ctx.cells(_records(occ, ids, dtype), occ.shape)
        for factor in FACTORS:
            R.assert_threshold_is_clear(occ, ids, extrema, factor * res)
            want = R.segment_labels_flood(occ, ids, extrema, factor * res)
            assert _same(cells.spatial_segments(extrema, factor * res), want), (occ.shape, factor)
        cells.close()


def test_spatial_segments_on_synthetic_extrema_128(ctx):
    import torch
    shape = (128, 128, 128)
    res = 0.125
    rng = np.random.default_rng(31)
    occ = rng.choice(R.OCCUPANCY_VALUES, size=shape).astype(np.float32)
    coarse = rng.integers(0, 4, size=(16, 16, 16)).astype(np.uint32)
    ids = np.repeat(np.repeat(np.repeat(coarse, 8, 0), 8, 1), 8, 2)
    extrema = R.lattice_extrema(shape, res, seed=32)
    cells = ctx.cells(_records(occ, ids, capi.TAGGED_OBJECT_COMPONENT_CELL), shape)
    extrema_dev = torch.from_numpy(extrema).cuda()
    for factor in FACTORS:
        R.assert_threshold_is_clear(occ, ids, extrema, factor * res)
        want = R.segment_labels_fast(occ, ids, extrema, factor * res)
        assert want[1] > 1 or factor == FACTORS[-1]
        assert _same(cells.spatial_segments(extrema, factor * res), want), factor
        labels_dev = torch.zeros(shape, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        count = cells.spatial_segments_dev(extrema_dev.data_ptr(), factor * res, labels_dev.data_ptr())
        assert _same((labels_dev.cpu().numpy().view(np.uint32), count), want), factor
    cells.close()


@pytest.mark.parametrize("add_virtual_border", [False, True])
def test_spatial_segment_chain_on_the_tagged_fixture(ctx, sdf_tagged_cases, add_virtual_border):
    """Cells -> SDF -> local extrema -> segments step by step (the CPU side labels the SAME extrema map the device
    produced), and vgt_hip_cells_update_spatial_segments, which must give exactly the step-by-step result."""
    assert sdf_tagged_cases
    for name, case in sdf_tagged_cases.items():
        rec = tagged_records(case, capi.TAGGED_OBJECT_COMPONENT_CELL)
        occ, ids, res = case["occ"], case["ids"], float(case["res"])
        cells = ctx.cells(rec, rec.shape)
        for uif in (False, True):
            if add_virtual_border:
                sdf, _, _ = cells.sdf(res, (), uif, True)
            else:
                sdf, _, _ = cells.free_and_named_objects_sdf(res, uif, False)
            extrema = ctx.sdf_local_extrema_map(sdf, res)
            for factor in FACTORS:
                threshold = factor * res
                R.assert_threshold_is_clear(occ, ids, extrema, threshold)
                want = R.segment_labels_flood(occ, ids, extrema, threshold)
                assert _same(cells.spatial_segments(extrema, threshold), want), (name, uif, factor)
                got = cells.update_spatial_segments(threshold, res, unknown_is_filled=uif,
                                                    add_virtual_border=add_virtual_border)
                assert _same(got, want), (name, uif, factor)
        cells.close()


def test_spatial_segments_need_object_ids(ctx):
    occ = np.zeros((3, 3, 3), np.float32)
    cells = ctx.cells(_records(occ, None, capi.OCCUPANCY_COMPONENT_CELL), occ.shape, object_id_offset=-1)
    with pytest.raises(ValueError):
        cells.spatial_segments(np.zeros((3, 3, 3, 3)), 1.0)
    with pytest.raises(ValueError):
        cells.update_spatial_segments(1.0, 0.1)
    cells.close()


# ---- component surfaces ----
def test_surface_mask_small_grids(ctx):
    for occ, _ in _small_cases():
        labels, _ = R.occupancy_labels_fast(occ)
        for types in range(1, 8):
            got = ctx.component_surface_mask(occ, labels, types)
            assert got.dtype == bool and np.array_equal(got, R.surface_mask(occ, labels, types)), (occ.shape, types)


def test_surface_mask_256(ctx, large_cases):
    import torch
    occ, (labels, _) = large_cases["unknown_mix"]
    occ_dev = torch.from_numpy(occ).cuda()
    labels_dev = torch.from_numpy(labels.view(np.int32)).cuda()
    mask_dev = torch.zeros(LARGE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for types in range(1, 8):
        ctx.component_surface_mask_dev(occ_dev.data_ptr(), labels_dev.data_ptr(), LARGE, types, mask_dev.data_ptr())
        ctx.synchronize()
        assert np.array_equal(mask_dev.cpu().numpy().astype(bool), R.surface_mask(occ, labels, types)), types
