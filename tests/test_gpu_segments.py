"""(gpu) vgt_hip_cast_segments[_dev] against tests/segment_ref.py, the CPU restatement of the call: integer outputs
equal, hit_fraction and min_value bit-identical (NaN patterns included), through the host and the device entry point,
on the reference test's 1000 segments over a 40^3 scene and on the smallest grids at which the walk can go wrong
(tests/segment_cases.py)."""
import math

import numpy as np
import pytest

import segment_cases as C
import segment_ref as S
from voxelized_geometry_tools_amd import capi

pytestmark = pytest.mark.gpu

RES = C.FIXTURE_RESOLUTION


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fixture_walks():
    """The field-independent part of the restatement for the 1000 fixture segments, computed once."""
    return S.walks(C.FIXTURE_COUNTS, RES, C.fixture_segments())


def same_bits(a, b, as_uint):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(nan_a, nan_b) and \
        np.array_equal(a[~nan_a].view(as_uint), b[~nan_b].view(as_uint))


def assert_same(got, want, what):
    counts = np.bincount(got.status, minlength=4).tolist()
    print(what, "statuses", counts, "cells examined", int(got.cells_examined.sum()))
    assert got.status.dtype == np.uint8 and got.hit_index.dtype == np.int32 and got.cells_examined.dtype == np.int32
    assert np.array_equal(got.status, want.status), (what, counts, np.bincount(want.status, minlength=4).tolist())
    assert np.array_equal(got.hit_index, want.hit_index), what
    assert np.array_equal(got.cells_examined, want.cells_examined), what
    assert same_bits(got.hit_fraction, want.hit_fraction, np.uint64), what
    assert (got.min_value is None) == (want.min_value is None) and (got.min_index is None) == (want.min_index is None)
    if want.min_value is not None:
        assert same_bits(got.min_value, want.min_value, np.uint32), what
        assert np.array_equal(got.min_index, want.min_index), what


def cast_dev(ctx, field, res, segments, occupancy_for_sdf=None, with_min=False, **kw):
    """The device-pointer entry point; with occupancy_for_sdf straight after vgt_hip_sdf_dev, so that the field never
    visits the host."""
    import torch
    seg = torch.from_numpy(np.ascontiguousarray(segments, dtype=np.float64).reshape(-1, 6)).cuda()
    n = seg.shape[0]
    room = max(n, 1)  # (an empty tensor has no address, and `status` is a required pointer)
    out = {"status": torch.full((room,), 77, dtype=torch.uint8, device="cuda"),
           "hit_index": torch.empty(room, dtype=torch.int32, device="cuda"),
           "hit_fraction": torch.empty(room, dtype=torch.float64, device="cuda"),
           "cells_examined": torch.empty(room, dtype=torch.int32, device="cuda")}
    if with_min:
        out["min_value"] = torch.empty(room, dtype=torch.float32, device="cuda")
        out["min_index"] = torch.empty(room, dtype=torch.int32, device="cuda")
    if occupancy_for_sdf is not None:
        shape = occupancy_for_sdf.shape
        occ = torch.from_numpy(np.ascontiguousarray(occupancy_for_sdf, dtype=np.float32)).cuda()
        dev_field = torch.empty(shape, dtype=torch.float32, device="cuda")
        nbytes = capi.sdf_workspace_bytes(shape)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.sdf_dev(occ.data_ptr(), shape, res, dev_field.data_ptr(), ws.data_ptr(), nbytes)
    else:
        shape = field.shape
        dev_field = torch.from_numpy(np.ascontiguousarray(field, dtype=np.float32)).cuda()
        torch.cuda.synchronize()
    ctx.cast_segments_dev(dev_field.data_ptr(), shape, res, seg.data_ptr(), n, out["status"].data_ptr(),
                          **{name + "_ptr": t.data_ptr() for name, t in out.items() if name != "status"}, **kw)
    ctx.synchronize()
    got = {name: t.cpu().numpy()[:n] for name, t in out.items()}
    return capi.SegmentCasts(got["status"], got["hit_index"], got["hit_fraction"], got["cells_examined"],
                             got.get("min_value"), got.get("min_index"))


def both_ways(ctx, field, res, segments, want, what, grid_from_world=None, **kw):
    with_min = want.min_value is not None
    assert_same(ctx.cast_segments(field, res, segments, with_min=with_min, grid_from_world=grid_from_world, **kw), want,
                what + " (host)")
    assert_same(cast_dev(ctx, field, res, segments, with_min=with_min, grid_from_world=grid_from_world, **kw), want,
                what + " (dev)")


@pytest.mark.parametrize("unknown_is_filled", [True, False])
def test_fixture_segments_through_occupancy(ctx, fixture_walks, unknown_is_filled):
    occ, seg = C.fixture_occupancy(), C.fixture_segments()
    for walk_through in (False, True):
        want = S.cast(occ, RES, seg, unknown_is_filled=unknown_is_filled, walk_through=walk_through, walked=fixture_walks)
        assert all(np.any(want.status == s) for s in (S.CLEAR, S.HIT, S.MISSED_GRID))
        both_ways(ctx, occ, RES, seg, want, "occupancy uif=%s through=%s" % (unknown_is_filled, walk_through),
                  unknown_is_filled=unknown_is_filled, walk_through=walk_through)


@pytest.fixture(scope="module")
def fixture_sdf(ctx):
    return ctx.sdf_from_occupancy(C.fixture_occupancy(), RES)[0]


@pytest.mark.parametrize("threshold", [-0.125, 0.0, 0.3])
@pytest.mark.parametrize("walk_through", [False, True])
def test_fixture_segments_through_the_sdf(ctx, fixture_walks, fixture_sdf, threshold, walk_through):
    seg = C.fixture_segments()
    want = S.cast(fixture_sdf, RES, seg, mode=S.SDF_BELOW, threshold=threshold, walk_through=walk_through, with_min=True,
                  walked=fixture_walks)
    assert all(np.any(want.status == s) for s in (S.CLEAR, S.HIT, S.MISSED_GRID))
    what = "sdf threshold=%g through=%s" % (threshold, walk_through)
    kw = dict(mode=capi.SEGMENT_SDF_BELOW, threshold=threshold, walk_through=walk_through)
    assert_same(ctx.cast_segments(fixture_sdf, RES, seg, with_min=True, **kw), want, what + " (host)")
    # the device entry point straight after vgt_hip_sdf_dev
    assert_same(cast_dev(ctx, None, RES, seg, occupancy_for_sdf=C.fixture_occupancy(), with_min=True, **kw), want,
                what + " (dev after sdf_dev)")
    # without the min outputs another kernel instantiation runs: the other outputs are the same
    plain = ctx.cast_segments(fixture_sdf, RES, seg, **kw)
    assert plain.min_value is None
    assert_same(plain, want._replace(min_value=None, min_index=None), what + " (no min outputs)")


ODD_FIELDS = {
    "empty map's SDF, all +inf": np.full(C.FIXTURE_COUNTS, math.inf, dtype=np.float32),
    "filled map's SDF, all -inf": np.full(C.FIXTURE_COUNTS, -math.inf, dtype=np.float32),
}


def _field_with_nans():
    field = (np.indices(C.FIXTURE_COUNTS).sum(axis=0).astype(np.float32) - 40.0) * np.float32(0.05)
    rng = np.random.default_rng(11)
    field[rng.random(C.FIXTURE_COUNTS) < 0.3] = math.nan
    field[10:14, :, :] = math.nan
    return field


@pytest.mark.parametrize("name", list(ODD_FIELDS) + ["NaN cells on the path"])
def test_odd_sdf_fields(ctx, fixture_walks, name):
    field = ODD_FIELDS[name] if name in ODD_FIELDS else _field_with_nans()
    seg = C.fixture_segments()
    for threshold, walk_through in ((0.0, False), (0.25, True), (math.inf, False), (-math.inf, True)):
        want = S.cast(field, RES, seg, mode=S.SDF_BELOW, threshold=threshold, walk_through=walk_through, with_min=True,
                      walked=fixture_walks)
        both_ways(ctx, field, RES, seg, want, "%s threshold=%g through=%s" % (name, threshold, walk_through),
                  mode=capi.SEGMENT_SDF_BELOW, threshold=threshold, walk_through=walk_through)


def test_odd_occupancy_values(ctx, fixture_walks):
    """Occupancy NaN (never a hit), exactly 0.5, the floats next to 0.5, and infinities."""
    rng = np.random.default_rng(3)
    values = np.array([0.0, 0.5, np.nextafter(np.float32(0.5), np.float32(1)), np.nextafter(np.float32(0.5), np.float32(0)),
                       math.nan, math.inf, -math.inf, 1.0], dtype=np.float32)
    occ = values[rng.choice(len(values), size=C.FIXTURE_COUNTS, p=[0.72, 0.04, 0.04, 0.04, 0.08, 0.02, 0.02, 0.04])]
    seg = C.fixture_segments()
    for unknown_is_filled in (True, False):
        want = S.cast(occ, RES, seg, unknown_is_filled=unknown_is_filled, walked=fixture_walks)
        both_ways(ctx, occ, RES, seg, want, "odd occupancy uif=%s" % unknown_is_filled,
                  unknown_is_filled=unknown_is_filled)


@pytest.mark.parametrize("case", C.HAND_CASES, ids=[c[0] for c in C.HAND_CASES])
def test_hand_cases(ctx, case):
    name, counts, filled, segment, status, hit_cell, examined, fraction, cells = case
    field = C.hand_field(counts, filled)
    for got in (ctx.cast_segments(field, C.HAND_RESOLUTION, [segment]),
                cast_dev(ctx, field, C.HAND_RESOLUTION, [segment])):
        assert got.status[0] == status
        assert got.hit_index[0] == (-1 if hit_cell is None else C.linear(counts, hit_cell))
        assert got.cells_examined[0] == examined
        if fraction is None:
            assert math.isnan(got.hit_fraction[0])
        else:
            assert got.hit_fraction[0] == fraction
    if cells is not None:
        # the order of examination, through the first hit: fill the k-th cell and the cast stops there after k + 1 cells
        for k, cell in enumerate(cells):
            got = ctx.cast_segments(C.hand_field(counts, [cell]), C.HAND_RESOLUTION, [segment])
            assert (got.status[0], got.hit_index[0], got.cells_examined[0]) == (S.HIT, C.linear(counts, cell), k + 1)


@pytest.mark.parametrize("counts", C.DEGENERATE_COUNTS, ids=str)
def test_degenerate_grids(ctx, counts):
    occ, res, seg = C.degenerate_case(counts)
    walked = S.walks(counts, res, seg)
    for unknown_is_filled, walk_through in ((True, False), (False, True)):
        want = S.cast(occ, res, seg, unknown_is_filled=unknown_is_filled, walk_through=walk_through, walked=walked)
        both_ways(ctx, occ, res, seg, want, "grid %s" % (counts,), unknown_is_filled=unknown_is_filled,
                  walk_through=walk_through)
    sdf = ctx.sdf_from_occupancy(occ, res)[0]
    want = S.cast(sdf, res, seg, mode=S.SDF_BELOW, threshold=0.5 * res, walk_through=True, with_min=True, walked=walked)
    both_ways(ctx, sdf, res, seg, want, "grid %s sdf" % (counts,), mode=capi.SEGMENT_SDF_BELOW, threshold=0.5 * res,
              walk_through=True)


def test_rotated_and_translated_frame(ctx):
    occ = C.fixture_occupancy()
    grid_from_world, world_from_grid = C.rotated_frame()
    seg = C.to_world(C.fixture_segments()[:300], world_from_grid)
    want = S.cast(occ, RES, seg, grid_from_world=grid_from_world)
    assert all(np.any(want.status == s) for s in (S.CLEAR, S.HIT, S.MISSED_GRID))
    both_ways(ctx, occ, RES, seg, want, "rotated frame", grid_from_world=grid_from_world)
    # an identity matrix is multiplied through, NULL is not: both give what the restatement gives for them
    identity = np.eye(4).reshape(16)
    seg = C.fixture_segments()[:300]
    both_ways(ctx, occ, RES, seg, S.cast(occ, RES, seg, grid_from_world=identity), "identity", grid_from_world=identity)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257])
def test_batch_sizes(ctx, fixture_walks, fixture_sdf, n):
    seg = C.fixture_segments()[:n].copy()
    walked = fixture_walks[:n]
    if n > 2:
        seg[1, 4] = math.nan     # an INVALID one in the batch
        walked = list(walked)
        walked[1] = None
    want = S.cast(fixture_sdf, RES, seg, mode=S.SDF_BELOW, threshold=0.1, with_min=True, walked=walked)
    both_ways(ctx, fixture_sdf, RES, seg, want, "batch of %d" % n, mode=capi.SEGMENT_SDF_BELOW, threshold=0.1)
    if n > 2:
        assert want.status[1] == S.INVALID and want.cells_examined[1] == 0 and want.min_index[1] == -1


def test_every_optional_output_may_be_null(ctx, fixture_walks, fixture_sdf):
    seg = np.ascontiguousarray(C.fixture_segments()[:257])
    n = len(seg)
    want = S.cast(fixture_sdf, RES, seg, mode=S.SDF_BELOW, threshold=0.1, with_min=True, walked=fixture_walks[:n])
    field = np.ascontiguousarray(fixture_sdf, dtype=np.float32)
    names = ["hit_index", "hit_fraction", "cells_examined", "min_value", "min_index"]
    for absent in names + [None]:
        buffers = {"hit_index": np.full(n, 9, np.int32), "hit_fraction": np.full(n, 7.0), "cells_examined": np.full(n, 9, np.int32),
                   "min_value": np.full(n, 7.0, np.float32), "min_index": np.full(n, 9, np.int32)}
        status = np.full(n, 9, np.uint8)
        capi.check(ctx._lib.vgt_hip_cast_segments(
            ctx.handle, capi._ptr(field), *field.shape, RES, capi.SEGMENT_SDF_BELOW, 1, 0.1, 0, None, capi._ptr(seg), n,
            capi._ptr(status), *[None if name == absent else capi._ptr(buffers[name]) for name in names]))
        got = capi.SegmentCasts(status, *[getattr(want, name) if name == absent else buffers[name] for name in names])
        assert_same(got, want, "without %s" % absent)
