"""(not gpu) The CPU yardsticks of the component labelling (tests/components_ref.py): the literal flood fill reproduces
labellings derived by hand, and the fast labelling equals the flood fill on them and on seeded random grids -- which is
what entitles the GPU tests to use the fast one on grids the flood fill is too slow for."""
import numpy as np
import pytest

import components_ref as R


@pytest.mark.parametrize("case", R.hand_cases(), ids=lambda c: c[0])
def test_flood_fill_reproduces_hand_derived_labels(case):
    _, occ, want, count = case
    got, n = R.occupancy_labels_flood(occ)
    assert got.dtype == np.uint32 and np.array_equal(got, want) and n == count
    fast, fn = R.occupancy_labels_fast(occ)
    assert np.array_equal(fast, want) and fn == count


def test_numbering_order_case_has_a_small_first_component():
    _, occ, want, _ = [c for c in R.hand_cases() if c[0] == "numbering_order"][0]
    assert np.count_nonzero(want == 1) < np.count_nonzero(want == 2) and want.reshape(-1)[0] == 1


def test_fast_labels_equal_the_flood_fill_on_random_grids():
    grids = R.random_small_grids(200)
    assert len(grids) == 200
    seen_nan = False
    for occ, ids in grids:
        assert all(1 <= s <= 12 for s in occ.shape)
        seen_nan |= bool(np.isnan(occ).any())
        for use_ids in (None, ids):
            want, count = R.occupancy_labels_flood(occ, use_ids)
            got, n = R.occupancy_labels_fast(occ, use_ids)
            assert np.array_equal(got, want) and n == count, occ.shape
            assert count == int(want.max())
    assert seen_nan


def test_fast_segment_labels_equal_the_flood_fill():
    res = 0.25
    for k, (occ, ids) in enumerate(R.random_small_grids(40, seed=77)):
        extrema = R.lattice_extrema(occ.shape, res, seed=1000 + k)
        for factor in (0.5, 1.75, 3.3, 1000.0):
            threshold = factor * res
            R.assert_threshold_is_clear(occ, ids, extrema, threshold)
            want, count = R.segment_labels_flood(occ, ids, extrema, threshold)
            got, n = R.segment_labels_fast(occ, ids, extrema, threshold)
            assert np.array_equal(got, want) and n == count
            assert np.array_equal(want == 0, ~R.segment_active(occ, ids, extrema))


def test_surface_rule_on_a_hand_case():
    # 5x5x5 all empty with one component: only the faces are surface cells
    occ = np.zeros((5, 5, 5), np.float32)
    labels = np.ones((5, 5, 5), np.uint32)
    mask = R.surface_mask(occ, labels, R.EMPTY_COMPONENTS)
    assert not mask[1:4, 1:4, 1:4].any() and mask.sum() == 125 - 27
    assert not R.surface_mask(occ, labels, R.FILLED_COMPONENTS | R.UNKNOWN_COMPONENTS).any()
    # a filled centre: the centre and its six face neighbours become surface cells, the 20 other inner cells do not
    occ[2, 2, 2] = 1.0
    labels[2, 2, 2] = 2
    mask = R.surface_mask(occ, labels, 7)
    assert mask[2, 2, 2] and mask[1, 2, 2] and mask[2, 2, 3] and not mask[1, 1, 1] and not mask[1, 1, 2]
    assert mask[1:4, 1:4, 1:4].sum() == 7
    assert R.surface_mask(occ, labels, R.FILLED_COMPONENTS).sum() == 1
    # NaN counts as unknown
    occ[2, 2, 2] = np.nan
    assert R.surface_mask(occ, labels, R.UNKNOWN_COMPONENTS).sum() == 1
