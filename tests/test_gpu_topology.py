"""(gpu) Component topology on the device against the CPU yardstick tests/topology_ref.topology_fast (itself shown equal
to the literal one in tests/test_topology_ref.py).  Every comparison is equality of all eight int32 fields of every
entry of the table, and of the labels where they are returned."""
import numpy as np
import pytest

import components_ref as R
import topology_ref as T
from test_gpu_components import LARGE, large_cases  # noqa: F401  (the 256^3 grids and their labels, read-only)
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _check(ctx, occ, types=7, tag=None):
    """Host entry point, twice on the same context: both tables equal the yardstick's; the labels are the labelling's."""
    occ, labels, count = T.labelled(occ)
    want = T.topology_fast(occ, labels, types, count)
    got, got_labels = ctx.component_topology(occ, types, with_labels=True)
    assert got.dtype == capi.COMPONENT_TOPOLOGY and T.tables_equal(got, want), (tag, occ.shape, types)
    assert np.array_equal(got_labels, labels), (tag, occ.shape)
    again = ctx.component_topology(occ, types)
    assert T.tables_equal(again, got), (tag, "second run differs")
    return got, labels


def test_known_answers(ctx):
    for name, occ, want in T.known_answer_cases():
        table, labels = _check(ctx, occ, 7, name)
        for cell, (holes, voids) in want.items():
            entry = table[labels[cell]]
            assert entry["present"] == 1 and (entry["num_holes"], entry["num_voids"]) == (holes, voids), (name, cell)


def test_hand_cases_every_component_type(ctx):
    for name, occ, _ in T.hand_cases():
        for types in range(1, 8):
            _check(ctx, occ, types, name)


def test_random_small_grids(ctx):
    grids = R.random_small_grids(200)
    assert len(grids) == 200
    for k, (occ, _) in enumerate(grids):
        _check(ctx, occ, 7, k)
        _check(ctx, occ, 1 + k % 7, k)


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 70, 1), (3, 5, 129), (65, 64, 63)])
def test_extents(ctx, shape):
    rng = np.random.default_rng(sum(shape))
    _check(ctx, rng.choice(R.OCCUPANCY_VALUES, size=shape).astype(np.float32), 7, "noise")
    blocks = rng.choice(np.array([0.0, 0.5, 1.0], np.float32), size=tuple((s + 3) // 4 for s in shape))
    occ = np.repeat(np.repeat(np.repeat(blocks, 4, 0), 4, 1), 4, 2)[:shape[0], :shape[1], :shape[2]].copy()
    for types in range(1, 8):
        _check(ctx, occ, types, "blocks")
    _check(ctx, np.ones(shape, np.float32), 7, "filled")


@pytest.mark.parametrize("p", [0.01, 0.3, 0.5])
def test_salt_96(ctx, p):
    """Many tiny components: the contended counters and the many-label path."""
    rng = np.random.default_rng(int(p * 100))
    occ = (rng.random((96, 96, 96)) < p).astype(np.float32)
    table, _ = _check(ctx, occ, 7, "salt %g" % p)
    assert len(table) > 5000
    _check(ctx, occ, 1, "salt %g filled" % p)


def test_spheres_256_on_the_device_after_the_labelling(ctx, large_cases):  # noqa: F811
    """Few huge components (the wave-reduced counters), and the _dev entry point chained after
    vgt_hip_connected_components_dev without a host round trip."""
    import torch
    occ, (labels, count) = large_cases["spheres"]
    occ_dev = torch.from_numpy(occ).cuda()
    labels_dev = torch.zeros(LARGE, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert ctx.connected_components_dev(occ_dev.data_ptr(), LARGE, labels_dev.data_ptr()) == count
    tables = {}
    for types in (7, 1, 2):
        want = T.topology_fast(occ, labels, types, count)
        for run in range(2):
            got = ctx.component_topology_dev(occ_dev.data_ptr(), labels_dev.data_ptr(), LARGE, types, count)
            assert T.tables_equal(got, want), (types, run)
        tables[types] = want
    assert np.array_equal(labels_dev.cpu().numpy().view(np.uint32), labels)      # (the input is not written)
    assert tables[7]["num_surface_vertices"].max() > 100000
    # the host entry point on the same grid
    got = ctx.component_topology(occ, 7)
    assert T.tables_equal(got, tables[7])


def test_dev_entry_point_small_and_foreign_labels(ctx):
    """Labels 0 and labels above num_components are "another component" and get no entry."""
    import torch
    rng = np.random.default_rng(77)
    occ = rng.choice(np.array([0.0, 1.0], np.float32), size=(9, 10, 11))
    occ, labels, count = T.labelled(occ)
    keep = max(1, count // 2)
    cut = np.where(labels <= keep, labels, np.where(labels % 2 == 0, 0, labels)).astype(np.uint32)
    occ_dev = torch.from_numpy(occ).cuda()
    labels_dev = torch.from_numpy(cut.view(np.int32)).cuda()
    torch.cuda.synchronize()
    got = ctx.component_topology_dev(occ_dev.data_ptr(), labels_dev.data_ptr(), occ.shape, 7, keep)
    assert T.tables_equal(got, T.topology_fast(occ, cut, 7, keep))


@pytest.mark.parametrize("dtype,offset", [(capi.OCCUPANCY_COMPONENT_CELL, -1), (capi.TAGGED_OBJECT_CELL, 4),
                                          (capi.TAGGED_OBJECT_COMPONENT_CELL, 4)], ids=["component8", "tagged8", "tagged16"])
def test_cells_with_and_without_connect_across_objects(ctx, dtype, offset):
    cases = [(occ, ids) for _, occ, ids in T.hand_cases()] + R.random_small_grids(60, seed=99)
    for k, (occ, ids) in enumerate(cases):
        rec = np.zeros(occ.shape, dtype=dtype)
        rec["occupancy"] = occ
        if "object_id" in dtype.names:
            rec["object_id"] = ids
        if "component" in dtype.names:
            rec["component"] = 0xABCD0123          # what the cells hold before must not matter
        cells = ctx.cells(rec, occ.shape, object_id_offset=offset)
        for across in (True, False):
            by_object = offset >= 0 and not across
            _, labels, count = T.labelled(occ, ids if by_object else None)
            types = 7 if k % 2 else 1 + k % 7
            want = T.topology_fast(occ, labels, types, count)
            got, got_labels = cells.component_topology(types, connect_across_objects=across, with_labels=True)
            assert T.tables_equal(got, want) and np.array_equal(got_labels, labels), (k, occ.shape, across, types)
            assert T.tables_equal(cells.component_topology(types, connect_across_objects=across), got)
        cells.close()


def test_table_capacity(ctx):
    """Too small a table is an error that still reports the number of components, and writes nothing."""
    import ctypes
    occ = np.zeros((4, 4, 4), np.float32)
    occ[1, 1, 1] = occ[2, 2, 2] = 1.0
    table = np.zeros(3, capi.COMPONENT_TOPOLOGY)
    count = ctypes.c_uint32(0)
    lib = ctx._lib
    rc = lib.vgt_hip_component_topology(ctx.handle, capi._ptr(occ), 4, 4, 4, 7, None, ctypes.byref(count),
                                        capi._ptr(table), 3)
    assert rc == 1 and count.value == 3 and b"4 entries" in lib.vgt_hip_last_error()
    assert not any(table[f].any() for f in table.dtype.names)
    assert len(ctx.component_topology(occ, 7)) == 4
    big = (np.random.default_rng(1).random((20, 20, 20)) < 0.3).astype(np.float32)     # more than the wrapper's first guess
    assert len(ctx.component_topology(big, 7)) > 257
