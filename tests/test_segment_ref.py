"""(not gpu) tests/segment_ref.py, the CPU restatement of vgt_hip_cast_segments that the device is compared against
(tests/test_gpu_segments.py), pinned by the oracle's f64 walk, by geometry and by answers written out by hand."""
import math

import numpy as np
import pytest

import segment_cases as C
import segment_ref as S


@pytest.fixture(scope="module")
def walks():
    """Per fixture segment: (the walk with the divergence rule, the reference's walk as it is)."""
    return [(S.walk(s[:3], s[3:], C.FIXTURE_COUNTS, C.FIXTURE_RESOLUTION),
             S.walk(s[:3], s[3:], C.FIXTURE_COUNTS, C.FIXTURE_RESOLUTION, divergence=False))
            for s in _fixture_as_the_oracle_sees_it()]


def _fixture_as_the_oracle_sees_it():
    """The oracle takes the point relative to the origin and adds the origin back: the segment's end is fl(p + origin)."""
    seg = C.fixture_segments().copy()
    seg[:, 3:] = (seg[:, 3:] - seg[:, :3]) + seg[:, :3]
    return seg


def test_cells_equal_the_oracles_walk(walks):
    """The set of cells of the restatement (without the divergence rule) = the cells raycast_f64 marks for the single
    point p = point - origin under a pure translation, max_range = inf."""
    from oracle import oracle as O
    vs = C.FIXTURE_RESOLUTION
    sizes = [c * vs for c in C.FIXTURE_COUNTS]
    mismatches = 0
    for ray, (_, reference) in zip(C.fixture_segments(), walks):
        origin, point = ray[:3], ray[3:]
        xf = np.eye(4)
        xf[:3, 3] = origin
        marked = O.raycast_f64((point - origin).reshape(1, 3), math.inf, xf.T.reshape(16), vs, 1.0 / vs, sizes,
                               C.FIXTURE_COUNTS)
        want = set(map(tuple, np.argwhere(marked.sum(axis=3) > 0).tolist()))
        assert marked.max() <= 1
        mismatches += want != set(reference.cells)
    print("walks that differ from the oracle's:", mismatches)
    assert mismatches == 0


def _boxes_meet_segment(lo, hi, a, b):
    """Slab test of the closed boxes [lo, hi] ([N, 3] each) against the segment a -> b, in plain doubles -> [N] bool."""
    t0, t1 = np.zeros(len(lo)), np.ones(len(lo))
    meets = np.ones(len(lo), dtype=bool)
    for k in range(3):
        d = b[k] - a[k]
        if d == 0.0:
            meets &= (a[k] >= lo[:, k]) & (a[k] <= hi[:, k])
        else:
            ta, tb = (lo[:, k] - a[k]) / d, (hi[:, k] - a[k]) / d
            t0, t1 = np.maximum(t0, np.minimum(ta, tb)), np.minimum(t1, np.maximum(ta, tb))
    return meets & (t0 <= t1)


def test_cells_are_the_cells_on_the_segment(walks):
    """Sound and complete for the segments the divergence rule keeps: every examined cell's box, grown by 1e-9, meets
    the segment; every in-grid cell whose box, shrunk by 1e-6, meets the segment is examined; no cell twice."""
    vs = C.FIXTURE_RESOLUTION
    top = np.array(C.FIXTURE_COUNTS) - 1
    must, missed = 0, 0
    for s, (kept, _) in zip(_fixture_as_the_oracle_sees_it(), walks):
        a, b = s[:3], s[3:]
        assert len(set(kept.cells)) == len(kept.cells)
        if kept.ended_before:
            assert kept.cells == []
            continue
        if kept.cells:
            cells = np.array(kept.cells, dtype=np.float64)
            assert np.all(_boxes_meet_segment(cells * vs - 1e-9, (cells + 1) * vs + 1e-9, a, b)), s
        # candidates: the cells of the segment's bounding box inside the grid
        low = np.clip(np.floor(np.minimum(a, b) / vs).astype(int), 0, top)
        high = np.clip(np.floor(np.maximum(a, b) / vs).astype(int), 0, top)
        box = np.stack(np.meshgrid(*[np.arange(low[k], high[k] + 1) for k in range(3)], indexing="ij"), axis=-1)
        box = box.reshape(-1, 3)
        on_segment = box[_boxes_meet_segment(box * vs + 1e-6, (box + 1) * vs - 1e-6, a, b)]
        examined = set(kept.cells)
        must += len(on_segment)
        missed += sum(tuple(cell) not in examined for cell in on_segment.tolist())
    print("cells that must be examined:", must, "missed:", missed)
    assert must == 27967
    assert missed == 0


def test_divergence_counts(walks):
    ended_before = [(kept, reference) for kept, reference in walks if reference.ended_before]
    would_examine = sum(1 for _, reference in ended_before if reference.cells)
    short_among_the_rest = sum(1 for kept, reference in walks if not reference.ended_before and kept.ended_short)
    short_in_all = sum(1 for _, reference in walks if reference.ended_short)
    print("segments that end before the grid:", len(ended_before), "of which the reference's walk examines cells:",
          would_examine, "walks ended short:", short_in_all, "among the rest:", short_among_the_rest)
    assert len(ended_before) == 142
    assert would_examine == 12
    assert short_in_all == 4
    assert short_among_the_rest == 0
    assert all(kept.cells == [] and kept.ended_before for kept, _ in ended_before)
    assert all(kept == reference for kept, reference in walks if not reference.ended_before)


@pytest.mark.parametrize("case", C.HAND_CASES, ids=[c[0] for c in C.HAND_CASES])
def test_hand_cases(case):
    name, counts, filled, segment, status, hit_cell, examined, fraction, cells = case
    field = C.hand_field(counts, filled)
    got = S.cast(field, C.HAND_RESOLUTION, [segment])
    assert got.status[0] == status
    assert got.hit_index[0] == (-1 if hit_cell is None else C.linear(counts, hit_cell))
    assert got.cells_examined[0] == examined
    if fraction is None:
        assert math.isnan(got.hit_fraction[0])
    else:
        assert got.hit_fraction[0] == fraction
    if cells is not None:
        assert S.walk(segment[:3], segment[3:], counts, C.HAND_RESOLUTION).cells == cells
        # the same cells whatever the field holds: walk-through examines them all
        through = S.cast(field, C.HAND_RESOLUTION, [segment], walk_through=True)
        assert through.cells_examined[0] == len(cells)


def test_fixture_scene_statuses():
    """What the GPU test relies on: each of CLEAR / HIT / MISSED_GRID occurs, and hits occur in the first and in the
    last examined cell."""
    occ, seg = C.fixture_occupancy(), C.fixture_segments()
    for unknown_is_filled, want, first_last in ((True, [291, 376, 333], (114, 13)), (False, [455, 212, 333], (98, 18))):
        got = S.cast(occ, C.FIXTURE_RESOLUTION, seg, unknown_is_filled=unknown_is_filled)
        through = S.cast(occ, C.FIXTURE_RESOLUTION, seg, unknown_is_filled=unknown_is_filled, walk_through=True)
        hits = got.status == S.HIT
        in_first = int(np.sum(hits & (got.cells_examined == 1)))
        in_last = int(np.sum(hits & (got.cells_examined == through.cells_examined)))
        print("unknown_is_filled", unknown_is_filled, np.bincount(got.status, minlength=3).tolist(), in_first, in_last)
        assert np.bincount(got.status, minlength=3).tolist() == want
        assert (in_first, in_last) == first_last
        assert np.array_equal(got.hit_index, through.hit_index) and np.array_equal(got.status, through.status)


def test_min_outputs_and_nan():
    """SDF mode on a hand-made field: NaN is never a hit and never a minimum, ties go to the first cell."""
    field = np.array([3.0, math.nan, 1.0, 1.0, math.inf, -math.inf], dtype=np.float32).reshape(1, 1, 6)
    up = (0.5, 0.5, 0.5, 0.5, 0.5, 5.5)
    got = S.cast(field, 1.0, [up], mode=S.SDF_BELOW, threshold=1.0, with_min=True)
    assert (got.status[0], got.hit_index[0], got.cells_examined[0], got.min_value[0], got.min_index[0]) == (1, 2, 3, 1.0, 2)
    got = S.cast(field, 1.0, [up], mode=S.SDF_BELOW, threshold=1.0, walk_through=True, with_min=True)
    assert (got.hit_index[0], got.cells_examined[0], got.min_value[0], got.min_index[0]) == (2, 6, -math.inf, 5)
    got = S.cast(field, 1.0, [up], mode=S.SDF_BELOW, threshold=0.5, walk_through=True, with_min=True)
    assert (got.status[0], got.hit_index[0], got.hit_fraction[0]) == (1, 5, 0.9)
    nans = np.full((1, 1, 3), math.nan, dtype=np.float32)
    got = S.cast(nans, 1.0, [(0.5, 0.5, 0.5, 0.5, 0.5, 2.5)], mode=S.SDF_BELOW, threshold=math.inf, with_min=True)
    assert (got.status[0], got.cells_examined[0], got.min_index[0]) == (0, 3, -1) and math.isnan(got.min_value[0])


def test_frame():
    """A rotated and shifted frame: the world-frame segments examine the cells of the grid-frame segments, up to
    the rounding of the transform (a few segments that graze a cell's corner may differ)."""
    occ, seg = C.fixture_occupancy(), C.fixture_segments()[:200]
    grid_from_world, world_from_grid = C.rotated_frame()
    direct = S.cast(occ, C.FIXTURE_RESOLUTION, seg)
    framed = S.cast(occ, C.FIXTURE_RESOLUTION, C.to_world(seg, world_from_grid), grid_from_world=grid_from_world)
    assert np.mean(direct.status == framed.status) > 0.97
    assert np.mean(direct.hit_index == framed.hit_index) > 0.97
