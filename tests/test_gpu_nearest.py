"""(gpu) The nearest-other-class transform (vgt_hip_nearest_*, vgt_hip_cells_nearest; contract in include/vgt_hip.h)
on the smallest grids at which each of its mechanisms can go wrong (tests/nearest_cases.py).  Every result goes through
the tolerant checker of tests/nearest_ref.py -- every cell, no index compared, so ties need no exemption --; the host,
mask and device entry points agree array for array, a second call repeats the first, the guard regions behind the
outputs stay untouched, and the squared distances reproduce the shipped SDF bit for bit."""
import numpy as np
import pytest

import nearest_cases as C
import nearest_ref as R
import sdf_conversion_ref
from conftest import bits_equal
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu

CASES = C.cases()
GUARD = 64
RES = 0.037


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def nearest_dev(ctx, occupancy, unknown_is_filled, with_d2=True):
    """The device entry point on buffers with a poisoned guard region behind the n cells: (nearest, d2)."""
    import torch
    occ = torch.from_numpy(np.ascontiguousarray(occupancy, dtype=np.float32)).cuda()
    n = occ.numel()
    nearest = torch.full((n + GUARD,), -77, dtype=torch.int32, device="cuda")
    d2 = torch.full((n + GUARD,), -78, dtype=torch.int32, device="cuda")
    nbytes = capi.nearest_workspace_bytes(occupancy.shape)
    assert nbytes >= 6 * n
    ws = torch.full((nbytes + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.nearest_dev(occ.data_ptr(), occupancy.shape, nearest.data_ptr(), ws.data_ptr(), nbytes,
                    d2_ptr=d2.data_ptr() if with_d2 else None, unknown_is_filled=unknown_is_filled)
    ctx.synchronize()
    nearest, d2, tail = nearest.cpu().numpy(), d2.cpu().numpy(), ws[nbytes:].cpu().numpy()
    assert (nearest[n:] == -77).all(), "the guard behind nearest was written"
    assert (d2[n:] == -78).all(), "the guard behind d2 was written"
    assert (tail == 0x5A).all(), "the guard behind the workspace was written"
    if not with_d2:
        assert (d2 == -78).all(), "d2 was written without being asked for"
    return nearest[:n].reshape(occupancy.shape), d2[:n].reshape(occupancy.shape)


@pytest.mark.parametrize("case", range(len(CASES)), ids=[c[0] for c in CASES])
def test_case(ctx, case):
    name, occ, unknown_is_filled = CASES[case]
    filled = C.filled_of(occ, unknown_is_filled)
    reference = R.reference_d2(filled)
    nearest, d2 = ctx.nearest_from_occupancy(occ, unknown_is_filled, with_d2=True)
    assert nearest.shape == occ.shape and d2.shape == occ.shape
    R.check(filled, nearest, d2, reference=reference)
    # the same call again, the call without d2, the mask and the device entry points: the same arrays
    again, d2_again = ctx.nearest_from_occupancy(occ, unknown_is_filled, with_d2=True)
    assert np.array_equal(again, nearest) and np.array_equal(d2_again, d2), "a second call differs"
    assert np.array_equal(ctx.nearest_from_occupancy(occ, unknown_is_filled), nearest)
    from_mask, d2_mask = ctx.nearest_from_mask(filled.astype(np.uint8) * 3, with_d2=True)
    assert np.array_equal(from_mask, nearest) and np.array_equal(d2_mask, d2), "the mask entry point differs"
    on_device, d2_device = nearest_dev(ctx, occ, unknown_is_filled)
    assert np.array_equal(on_device, nearest) and np.array_equal(d2_device, d2), "the device entry point differs"
    assert np.array_equal(nearest_dev(ctx, occ, unknown_is_filled, with_d2=False)[0], nearest)
    # the predicate and the distances are the shipped SDF's
    if filled.any() and not filled.all():
        want = sdf_conversion_ref.expected_sdf(d2.astype(np.float64), filled, RES)
        got = ctx.sdf_from_occupancy(occ, RES, unknown_is_filled, add_virtual_border=False)[0]
        assert bits_equal(got, want), sdf_conversion_ref.first_mismatch(got, want)
    else:
        assert (nearest == -1).all() and (d2 == 0x7fffffff).all()


@pytest.mark.parametrize("axis", range(3))
def test_longest_lines_in_closed_form(ctx, axis):
    shape = [1, 1, 1]
    shape[axis] = 16384
    occ = np.zeros(shape, dtype=np.float32)
    occ[0, 0, 0] = 1.0
    nearest, d2 = ctx.nearest_from_occupancy(occ, with_d2=True)
    i = np.arange(16384, dtype=np.int64)
    assert nearest.ravel()[0] == 1 and d2.ravel()[0] == 1
    assert (nearest.ravel()[1:] == 0).all()
    assert np.array_equal(d2.ravel()[1:].astype(np.int64), (i * i)[1:])


def test_odd_occupancy_values(ctx):
    """Non-finite and edge values are classed as vgt_hip_sdf_dev classes them."""
    values = np.array([np.nan, np.inf, -np.inf, 0.5, np.nextafter(np.float32(0.5), np.float32(1)),
                       np.nextafter(np.float32(0.5), np.float32(0)), -0.0, 1e-45, 3e38, 0.0, 1.0], dtype=np.float32)
    occ = values[np.random.RandomState(3).randint(0, values.size, size=(9, 7, 70))]
    for unknown_is_filled in (True, False):
        filled = C.filled_of(occ, unknown_is_filled)
        nearest, d2 = ctx.nearest_from_occupancy(occ, unknown_is_filled, with_d2=True)
        R.check(filled, nearest, d2)
        want = sdf_conversion_ref.expected_sdf(d2.astype(np.float64), filled, RES)
        assert bits_equal(ctx.sdf_from_occupancy(occ, RES, unknown_is_filled, add_virtual_border=False)[0], want)


@pytest.mark.parametrize("dtype", [capi.TAGGED_OBJECT_CELL, capi.TAGGED_OBJECT_COMPONENT_CELL], ids=["tagged8", "tagged16"])
def test_tagged_cells(ctx, dtype):
    from oracle import oracle as O
    occ, ids = C.tagged_scene()
    rec = np.zeros(occ.shape, dtype=dtype)
    rec["occupancy"], rec["object_id"] = occ, ids
    if "component" in dtype.names:
        rec["component"], rec["spatial_segment"] = 7, 0xDEADBEEF
    cells = ctx.cells(rec, rec.shape)
    for objects, unknown_is_filled in (((), True), ((), False), ((1, 3), True), ((2, 2, 0), False), ((99,), True)):
        mask = O.cells_filled_mask(rec, rec.shape, 1 if objects else 0, objects, unknown_is_filled).astype(bool)
        nearest, d2, obj = cells.nearest(objects, unknown_is_filled, with_d2=True, with_object_ids=True)
        R.check(mask, nearest, d2)
        assert obj.dtype == np.uint32 and obj.shape == occ.shape
        flat_ids = ids.ravel()
        want = np.where(mask.ravel(), flat_ids, np.where(nearest.ravel() >= 0, flat_ids[np.maximum(nearest.ravel(), 0)], 0))
        assert np.array_equal(obj.ravel(), want.astype(np.uint32))
        assert np.array_equal(cells.nearest(objects, unknown_is_filled), nearest)
        if mask.any():
            # every free cell is labelled with an object that has filled cells (the partition of free space)
            assert set(np.unique(obj[~mask])) <= set(np.unique(ids[mask]))
            assert np.array_equal(ctx.nearest_from_mask(mask.astype(np.uint8)), nearest)
        else:
            assert (nearest == -1).all() and (obj == 0).all()
    cells.close()
    # a cell type without object ids: the transform works, the object output is refused
    plain = np.zeros(occ.shape, dtype=capi.OCCUPANCY_COMPONENT_CELL)
    plain["occupancy"] = occ
    cells = ctx.cells(plain, plain.shape, object_id_offset=-1)
    R.check(C.filled_of(occ), cells.nearest())
    with pytest.raises(ValueError, match="no object id"):
        cells.nearest(with_object_ids=True)
    cells.close()
