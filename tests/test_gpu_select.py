"""(gpu) The cell selection on the device against tests/select_ref.py: indices, their order, values and labels are
compared bit for bit (np.array_equal on int32 / uint32 views) for every rule and every non-empty class mask."""
import ctypes

import numpy as np
import pytest

import select_cases as C
import select_ref as R
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu

RULES = (R.SELECT_ALL, R.SELECT_SURFACE_26, R.SELECT_COMPONENT_SURFACE)
MASKS = range(1, 16)
SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(got, want):
    """(indices, values, labels) against the reference's, bit for bit."""
    return got[0].dtype == np.int32 and np.array_equal(got[0], want[0]) and \
        np.array_equal(_bits(got[1]), _bits(want[1])) and np.array_equal(got[2], want[2])


class DeviceGrid:
    """A value and a label grid on the device, with output lists of the grid's size and a sentinel fill."""

    def __init__(self, torch, values, labels):
        self.torch = torch
        self.shape = values.shape
        self.n = values.size
        self.values = torch.from_numpy(np.ascontiguousarray(values)).cuda()
        self.labels = torch.from_numpy(np.ascontiguousarray(labels).view(np.int32)).cuda()
        self.out = torch.full((3, self.n), SENTINEL, dtype=torch.int32, device="cuda")

    def ptrs(self):
        return [self.out[k].data_ptr() for k in range(3)]

    def run(self, ctx, rule, mask, threshold=0.5, capacity=None):
        i, v, l = self.ptrs()
        return ctx.select_cells_dev(self.values.data_ptr(), self.shape, rule, mask, threshold, self.labels.data_ptr(),
                                    i, v, l, self.n if capacity is None else capacity)

    def lists(self, count):
        host = self.out[:, :count].cpu().numpy()
        return host[0].copy(), host[1].view(np.float32).copy(), host[2].view(np.uint32).copy()


@pytest.mark.parametrize("shape", C.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_rule_and_class_mask(ctx, torch, shape):
    n = int(np.prod(shape))
    counts = set()
    for name, (values, labels) in C.value_sets(shape, seed=sum(shape)).items():
        grid = DeviceGrid(torch, values, labels)
        class_grid = R.classes(values, 0.5)
        for rule in RULES:
            rule_grid = R.rule_mask(values, rule, labels)
            for mask in MASKS:
                want = R.select(values, rule, mask, 0.5, labels, rule_grid, class_grid)
                count = grid.run(ctx, rule, mask)
                assert count == len(want[0]), (name, rule, mask)
                assert _same(grid.lists(count), want), (name, rule, mask)
                counts.add((name, count))
    assert ("uniform", 0) in counts and ("everything", n) in counts


@pytest.mark.parametrize("shape", C.SMALL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_host_entry_point(ctx, shape):
    values, labels = C.value_sets(shape, seed=5)["random"]
    for rule in RULES:
        for mask in MASKS:
            want = R.select(values, rule, mask, 0.5, labels)
            got = ctx.select_cells(values, rule, mask, labels=labels, with_values=True, with_labels=True)
            assert _same(got, want), (rule, mask)
            if rule != R.SELECT_COMPONENT_SURFACE:
                only = ctx.select_cells(values, rule, mask)
                assert only.dtype == np.int32 and np.array_equal(only, want[0])


@pytest.mark.parametrize("shape", [(3, 3, 3), (2, 3, 65), (5, 7, 130), (40, 33, 70)], ids=lambda s: "x".join(map(str, s)))
def test_sdf_threshold_zero(ctx, shape):
    field = C.sdf_field(shape, seed=11)
    assert np.signbit(field[field == 0]).any() and not np.signbit(field[field == 0]).all()
    with np.errstate(invalid="ignore"):
        want = np.flatnonzero((field <= 0).reshape(-1))
    got, values = ctx.select_cells(field, R.SELECT_ALL, R.CLASS_BELOW | R.CLASS_EQUAL, threshold=0.0, with_values=True)
    assert np.array_equal(got, want)                                       # ExportSDFForDisplayCollisionOnly
    assert np.array_equal(_bits(values), _bits(field.reshape(-1)[want]))   # -0.0 stays -0.0
    for mask in MASKS:
        assert np.array_equal(ctx.select_cells(field, R.SELECT_ALL, mask, threshold=0.0),
                              R.select(field, R.SELECT_ALL, mask, 0.0)[0]), mask


def test_count_capacity_and_repeat(ctx, torch):
    shape = (5, 7, 130)
    values, labels = C.value_sets(shape, seed=2)["random"]
    grid = DeviceGrid(torch, values, labels)
    mask = 11                                                              # (not 15: SELECT_ALL must leave cells out)
    for rule in RULES:
        want = R.select(values, rule, mask, 0.5, labels)
        n = len(want[0])
        assert 1 < n < grid.n
        # count only
        assert ctx.select_cells_dev(grid.values.data_ptr(), shape, rule, mask, 0.5, grid.labels.data_ptr()) == n
        assert (grid.out == SENTINEL).all()
        # one entry short: an error naming both numbers, the true count, nothing written
        count = ctypes.c_int64(-1)
        i, v, l = grid.ptrs()
        rc = ctx._lib.vgt_hip_select_cells_dev(ctx.handle, grid.values.data_ptr(), grid.labels.data_ptr(), *shape, rule,
                                               mask, 0.5, i, v, l, n - 1, ctypes.byref(count))
        assert rc == 1 and count.value == n
        assert str(n) in capi.last_error() and str(n - 1) in capi.last_error()
        assert (grid.out == SENTINEL).all()
        with pytest.raises(ValueError):
            grid.run(ctx, rule, mask, capacity=n - 1)
        # exact capacity: the lists and nothing behind them
        assert grid.run(ctx, rule, mask, capacity=n) == n
        assert _same(grid.lists(n), want) and (grid.out[:, n:] == SENTINEL).all()
        first = grid.out.clone()
        grid.out.fill_(SENTINEL)
        assert grid.run(ctx, rule, mask, capacity=n) == n
        assert torch.equal(first, grid.out)                                # two runs, equal bytes
        grid.out.fill_(SENTINEL)


def test_callers_stream(ctx, torch):
    shape = (2, 3, 65)
    values, labels = C.value_sets(shape, seed=4)["random"]
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        grid = DeviceGrid(torch, values, labels)
    stream.synchronize()
    ctx.set_stream(stream.cuda_stream)
    try:
        for rule in RULES:
            want = R.select(values, rule, 15, 0.5, labels)
            count = grid.run(ctx, rule, 15)
            stream.synchronize()
            assert count == len(want[0]) and _same(grid.lists(count), want)
    finally:
        ctx.reset_stream()


# (record dtype or None = a plain float grid, object id offset, members the layout has)
LAYOUTS = [
    (None, -1, ()),
    (capi.OCCUPANCY_COMPONENT_CELL, -1, ("component",)),
    (capi.TAGGED_OBJECT_CELL, 4, ("object_id",)),
    (capi.TAGGED_OBJECT_COMPONENT_CELL, 4, ("object_id", "component", "spatial_segment")),
]
MEMBERS = {"object_id": capi.CELL_MEMBER_OBJECT_ID, "component": capi.CELL_MEMBER_COMPONENT,
           "spatial_segment": capi.CELL_MEMBER_SPATIAL_SEGMENT}


@pytest.mark.parametrize("layout", LAYOUTS, ids=["float4", "component8", "tagged8", "tagged16"])
def test_cells_select(ctx, torch, layout):
    dtype, id_offset, members = layout
    shape = (5, 7, 130)
    values, labels = C.value_sets(shape, seed=8)["random"]
    rng = np.random.default_rng(8)
    if dtype is None:
        records = values
    else:
        records = np.zeros(shape, dtype=dtype)
        records["occupancy"] = values
        for k, name in enumerate(members):
            records[name] = labels if name == "component" else rng.integers(0, 1 << 32, size=shape, dtype=np.uint32)
    cells = ctx.cells(records, shape, object_id_offset=id_offset)
    try:
        for rule in (R.SELECT_ALL, R.SELECT_SURFACE_26):
            for mask in (1, 6, 9, 15):
                want = R.select(values, rule, mask)
                got = cells.select(rule, mask)
                assert got.dtype == np.int32 and np.array_equal(got, want[0])
                for name in members:
                    got = cells.select(rule, mask, MEMBERS[name], with_occupancy=True)
                    assert np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
                    assert got[2].dtype == np.uint32 and np.array_equal(got[2], records[name].reshape(-1)[want[0]])
        # the component rule: the cells' own component member, or labels on the device
        want = R.select(values, R.SELECT_COMPONENT_SURFACE, 15, labels=labels)
        if "component" in members:
            got = cells.select(R.SELECT_COMPONENT_SURFACE, 15, capi.CELL_MEMBER_COMPONENT)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[2])
        else:
            with pytest.raises(ValueError):
                cells.select(R.SELECT_COMPONENT_SURFACE, 15)
        other = np.ascontiguousarray(labels[::-1, ::-1, ::-1])
        other_dev = torch.from_numpy(other.view(np.int32)).cuda()
        want = R.select(values, R.SELECT_COMPONENT_SURFACE, 7, labels=other)
        assert np.array_equal(cells.select(R.SELECT_COMPONENT_SURFACE, 7, labels_ptr=other_dev.data_ptr()), want[0])
        # members the layout does not have
        for name, member in MEMBERS.items():
            if name not in members:
                with pytest.raises(ValueError):
                    cells.select(R.SELECT_ALL, 15, member)
    finally:
        cells.close()
