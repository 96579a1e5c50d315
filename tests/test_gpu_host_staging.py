"""(gpu) The host-pointer entry points that stage through csrc/host_staging.hpp and have optional outputs, on a 3 x 5 x 7
grid (and 5 queries' worth of lists): the smallest shapes at which every array of a call ends off a 256-byte boundary,
so each later array lies at a carved address.  Each entry point is called once with all its optional outputs and once
with none: what it always returns must be byte-equal between the two and byte-equal to the device entry point fed the
same inputs.  (What the outputs should hold is the business of the entry points' own suites; the failure paths are run
on the CPU, tests/test_host_staging.py.)"""
import ctypes

import numpy as np
import pytest

from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu

SHAPE = (3, 5, 7)
N = 3 * 5 * 7
RES = 0.25


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def occupancy():
    """Filled, free and unknown cells, about a third each; at least two components of each class."""
    return np.random.default_rng(357).choice(np.array([0.0, 0.5, 1.0], np.float32), size=SHAPE)


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_coarse_gradient_with_and_without_has_value(ctx, torch):
    field = np.random.default_rng(1).normal(0.0, 1.0, SHAPE).astype(np.float32)
    with_has, has = ctx.sdf_coarse_gradient(field, RES, True)
    without = np.full(SHAPE + (3,), -7.0, dtype=np.float64)
    capi.check(ctx._lib.vgt_hip_sdf_coarse_gradient(ctx.handle, capi._ptr(field), *SHAPE, RES, 1, None, capi._ptr(without),
                                                    None))
    assert same_bytes(without, with_has)
    sdf_dev = torch.from_numpy(field).cuda()
    grad_dev = torch.zeros(SHAPE + (3,), dtype=torch.float64, device="cuda")
    has_dev = torch.zeros(SHAPE, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.sdf_coarse_gradient_dev(sdf_dev.data_ptr(), SHAPE, RES, grad_dev.data_ptr(), has_dev.data_ptr(), True)
    ctx.synchronize()
    assert same_bytes(grad_dev.cpu().numpy(), with_has)
    assert same_bytes(has_dev.cpu().numpy().astype(bool), has)
    assert has.any()  # (the comparison is not of two empty results)


def nearest_on_device(ctx, torch, occupancy, unknown_is_filled):
    occ_dev = torch.from_numpy(occupancy).cuda()
    nearest_dev = torch.full((N,), -77, dtype=torch.int32, device="cuda")
    nbytes = capi.nearest_workspace_bytes(SHAPE)
    ws_dev = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.nearest_dev(occ_dev.data_ptr(), SHAPE, nearest_dev.data_ptr(), ws_dev.data_ptr(), nbytes,
                    unknown_is_filled=unknown_is_filled)
    ctx.synchronize()
    return nearest_dev.cpu().numpy().reshape(SHAPE)


@pytest.mark.parametrize("unknown_is_filled", [True, False])
def test_nearest_with_and_without_d2(ctx, torch, occupancy, unknown_is_filled):
    with_d2, d2 = ctx.nearest_from_occupancy(occupancy, unknown_is_filled, with_d2=True)
    without = ctx.nearest_from_occupancy(occupancy, unknown_is_filled)
    assert same_bytes(without, with_d2)
    assert same_bytes(nearest_on_device(ctx, torch, occupancy, unknown_is_filled), with_d2)
    assert (with_d2 >= 0).all() and (d2 > 0).all()


def test_cells_nearest_with_and_without_d2_and_object(ctx, torch, occupancy):
    rec = np.zeros(SHAPE, dtype=capi.TAGGED_OBJECT_CELL)
    rec["occupancy"] = occupancy
    rec["object_id"] = np.arange(N, dtype=np.uint32).reshape(SHAPE) % 3 + 1
    cells = ctx.cells(rec, SHAPE)
    with_all, d2, obj = cells.nearest((), True, with_d2=True, with_object_ids=True)
    without = cells.nearest((), True)
    assert same_bytes(without, with_all)
    assert same_bytes(nearest_on_device(ctx, torch, occupancy, True), with_all)
    assert (d2 > 0).all() and set(np.unique(obj)) <= {1, 2, 3}
    # an object list, which goes through the handle's cached list and not through the staged block
    some, some_d2 = cells.nearest((2, 3), True, with_d2=True)
    assert same_bytes(cells.nearest((2, 3), True), some) and not same_bytes(some, with_all)
    cells.close()


def test_select_cells_with_and_without_value_and_label_lists(ctx, torch, occupancy):
    labels = (np.arange(N, dtype=np.uint32).reshape(SHAPE) * 2654435761 >> 7).astype(np.uint32)
    mask = capi.CLASS_ABOVE | capi.CLASS_EQUAL
    indices, values, picked = ctx.select_cells(occupancy, capi.SELECT_ALL, mask, labels=labels, with_values=True,
                                               with_labels=True)
    assert 5 < len(indices) < N and len(indices) % 64 != 0
    assert same_bytes(values, occupancy.ravel()[indices]) and same_bytes(picked, labels.ravel()[indices])
    # no optional list: with the labels given (they stay on the host: nothing needs them) and without
    assert same_bytes(ctx.select_cells(occupancy, capi.SELECT_ALL, mask, labels=labels), indices)
    assert same_bytes(ctx.select_cells(occupancy, capi.SELECT_ALL, mask), indices)
    values_dev = torch.from_numpy(occupancy).cuda()
    labels_dev = torch.from_numpy(labels.view(np.int32)).cuda()
    out_dev = torch.full((3, N), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    count = ctx.select_cells_dev(values_dev.data_ptr(), SHAPE, capi.SELECT_ALL, mask, 0.5, labels_dev.data_ptr(),
                                 out_dev[0].data_ptr(), out_dev[1].data_ptr(), out_dev[2].data_ptr(), N)
    out = out_dev.cpu().numpy()
    assert count == len(indices)
    assert same_bytes(out[0, :count], indices)
    assert same_bytes(out[1, :count].view(np.float32), values) and same_bytes(out[2, :count].view(np.uint32), picked)


def test_component_topology_with_and_without_labels(ctx, torch, occupancy):
    with_labels, labels = ctx.component_topology(occupancy, 7, with_labels=True)
    without = ctx.component_topology(occupancy, 7)
    count = len(with_labels) - 1
    assert count >= 6 and int(labels.max()) == count and int(labels.min()) == 1
    assert same_bytes(without, with_labels)
    occ_dev = torch.from_numpy(occupancy).cuda()
    labels_dev = torch.zeros(SHAPE, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert ctx.connected_components_dev(occ_dev.data_ptr(), SHAPE, labels_dev.data_ptr()) == count
    assert same_bytes(labels_dev.cpu().numpy().view(np.uint32), labels)
    assert same_bytes(ctx.component_topology_dev(occ_dev.data_ptr(), labels_dev.data_ptr(), SHAPE, 7, count), with_labels)
    # the capacity check between labelling and table: the count still comes back, the table and the labels stay
    num = ctypes.c_uint32(0)
    table = np.zeros(count, dtype=capi.COMPONENT_TOPOLOGY)
    kept = np.full(SHAPE, 0xEEEEEEEE, dtype=np.uint32)
    rc = ctx._lib.vgt_hip_component_topology(ctx.handle, capi._ptr(occupancy), *SHAPE, 7, capi._ptr(kept),
                                             ctypes.byref(num), capi._ptr(table), count)
    assert rc == 1 and num.value == count and str(count + 1) in capi.last_error()
    assert (kept == 0xEEEEEEEE).all() and not table.view(np.int32).any()
