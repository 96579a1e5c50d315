"""(not gpu) tests/filter_ref.py, the numpy restatement of the reference's combine-and-filter rule that the device is
compared against (tests/test_gpu_filter.py): bit-equal to the oracle library on every case family of
tests/filter_cases.py, and proof with the restatement alone that those inputs discriminate -- float against double in
both directions, `>=` against `>`, every output and a skipped cell per family, counts beyond the accumulate kernel's
launch cap."""
import numpy as np
import pytest

import filter_cases as C
import filter_ref as R
from conftest import bits_equal


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


def _runs(case):
    for option in case.options:
        for in_double in (False, True):
            yield option, in_double


@pytest.mark.parametrize("family", list(C.FAMILIES))
def test_restatement_equals_the_oracle(oracle, family):
    """... and the family reaches 0.0, 0.5 and 1.0 in both precisions and leaves a skipped cell's bits alone."""
    reached = {False: set(), True: set()}
    skipped_cells = 0
    for case in C.FAMILIES[family]():
        skipped = R.skipped(case.static)
        skipped_cells += int(skipped.sum())
        for (percent, outlier, cameras), in_double in _runs(case):
            got = R.filter_grids(case.tracking, case.static, percent, outlier, cameras, in_double)
            want = oracle.filter_grids(case.tracking, case.static, percent, outlier, cameras, in_double)
            assert bits_equal(got, want), (case.name, percent, outlier, cameras, in_double)
            assert bits_equal(got[skipped], case.static[skipped])
            assert set(np.unique(got[~skipped]).tolist()) <= {0.0, 0.5, 1.0}
            reached[in_double] |= set(np.unique(got[~skipped]).tolist())
    assert reached[False] == {0.0, 0.5, 1.0} and reached[True] == {0.0, 0.5, 1.0}
    assert skipped_cells >= 1


def test_large_grid_restatement_equals_the_oracle(oracle):
    """The grids one launch cannot cover (tests/test_gpu_filter.py): their pinned cells are unknown cells that every
    option changes, the first to 1.0 and the next to 0.0, and the cells around them are not all alike."""
    for threads in (C.DEFAULT_THREADS, C.SMALLEST_THREADS):
        cells = C.over_the_cap(threads)
        case = C.mixture(cells)
        marks = C.marked_cells(cells)
        assert marks[0] == cells - 1 and C.FILTER_MAX_WORKGROUPS * threads in marks
        assert not R.skipped(case.static)[marks].any()
        for (percent, outlier, cameras), in_double in _runs(case):
            got = R.filter_grids(case.tracking, case.static, percent, outlier, cameras, in_double)
            assert bits_equal(got, oracle.filter_grids(case.tracking, case.static, percent, outlier, cameras, in_double))
            assert got[marks].tolist() == [1.0, 0.0, 1.0][:len(marks)]
            tail = got[C.FILTER_MAX_WORKGROUPS * threads:]
            assert len(np.unique(tail)) >= 3 and (tail != case.static[C.FILTER_MAX_WORKGROUPS * threads:]).sum() > 100


def _verdicts(triples, in_double, strict=False):
    """Whether one camera holding (free, filled) is seen free at the triple's own threshold."""
    out = []
    for free, filled, percent in triples:
        saw_free, saw_filled = R.seen_as([free], [filled], percent, 1, in_double, strict)
        assert saw_free[0] != saw_filled[0]
        out.append(bool(saw_free[0]))
    return np.array(out)


def test_committed_triples_split_float_from_double():
    assert len(C.FLOAT_FREE_DOUBLE_FILLED) >= 8 and len(C.FLOAT_FILLED_DOUBLE_FREE) >= 8
    assert _verdicts(C.FLOAT_FREE_DOUBLE_FILLED, False).all() and not _verdicts(C.FLOAT_FREE_DOUBLE_FILLED, True).any()
    assert not _verdicts(C.FLOAT_FILLED_DOUBLE_FREE, False).any() and _verdicts(C.FLOAT_FILLED_DOUBLE_FREE, True).all()
    # the first direction needs no large count (all but its last triple), the second is made of them
    assert all(max(a, b) <= 12 for a, b, _ in C.FLOAT_FREE_DOUBLE_FILLED[:-1])
    assert all(max(a, b) >= 2 ** 24 - 1 for a, b, _ in C.FLOAT_FILLED_DOUBLE_FREE)
    assert all(0.0 < p <= 1.0 and a + b < 2 ** 30 for a, b, p in C.tie_triples())


def test_tie_family_disagrees_in_both_directions():
    """Over the family's runs, on its grid: at least 8 cells where the float rule gives free and the double rule filled,
    at least 8 the other way round, and the committed triples are among them."""
    (case,) = C.ties()
    triples = C.tie_triples()
    float_free, float_filled = 0, 0
    for percent, outlier, cameras in case.options:
        in_float = R.filter_grids(case.tracking, case.static, percent, outlier, cameras, False)
        in_double = R.filter_grids(case.tracking, case.static, percent, outlier, cameras, True)
        float_free += int(((in_float == 0.0) & (in_double == 1.0)).sum())
        float_filled += int(((in_float == 1.0) & (in_double == 0.0)).sum())
        for cell, (_, _, p) in enumerate(triples):
            if p != percent:
                continue
            if cell < len(C.FLOAT_FREE_DOUBLE_FILLED):
                assert (in_float[cell], in_double[cell]) == (0.0, 1.0)
            elif cell < len(C.FLOAT_FREE_DOUBLE_FILLED) + len(C.FLOAT_FILLED_DOUBLE_FREE):
                assert (in_float[cell], in_double[cell]) == (1.0, 0.0)
            else:
                assert (in_float[cell], in_double[cell]) == (0.0, 0.0)
    assert float_free >= 8 and float_filled >= 8, (float_free, float_filled)


def test_exact_ties_turn_on_the_comparison():
    """`>` in place of `>=` changes the exact ties and nothing else: the triples that tie in both precisions, in float
    the triples whose threshold rounds to the float ratio, in double the triples whose threshold is the double ratio."""
    both, first, second = C.TIES_IN_BOTH, C.FLOAT_FREE_DOUBLE_FILLED, C.FLOAT_FILLED_DOUBLE_FREE
    for in_double in (False, True):
        assert _verdicts(both, in_double).all() and not _verdicts(both, in_double, strict=True).any()
    assert not _verdicts(first, False, strict=True).any()         # float ties: free only by `>=`
    assert _verdicts(second, True).all() and not _verdicts(second, True, strict=True).any()     # double ties
    # far from a tie, the comparison's form does not matter
    loose = [(a, b, 0.47) for a in range(1, 13) for b in range(1, 13)]
    for in_double in (False, True):
        assert np.array_equal(_verdicts(loose, in_double), _verdicts(loose, in_double, strict=True))
    # and on the family's grid the filtered occupancy changes at those cells
    (case,) = C.ties()
    changed = 0
    for (percent, outlier, cameras), in_double in _runs(case):
        rule = R.filter_grids(case.tracking, case.static, percent, outlier, cameras, in_double)
        strict = R.filter_grids(case.tracking, case.static, percent, outlier, cameras, in_double, strict=True)
        changed += int((rule != strict).sum())
        assert ((rule == strict) | ((rule == 0.0) & (strict == 1.0))).all()
    assert changed >= len(both) * 2 + len(first) + len(second)


def test_ratio_sweep_thresholds():
    """Each reachable ratio is a threshold, with the double below and the double above it; in double the three differ
    on the cells of that ratio, in float they are one threshold."""
    (case,) = C.ratio_sweep()
    ratios = C.small_ratios()
    assert len(case.options) == 3 * len(ratios) and len(ratios) > 80
    cell = {(a, b): a * 13 + b for a in range(13) for b in range(13)}
    for a, b in ((3, 2), (1, 12), (12, 1), (7, 7), (5, 11)):
        r = a / (a + b)
        below, at, above = [R.filter_grids(case.tracking, case.static, p, 1, 1, True)[cell[a, b]]
                            for p in (np.nextafter(r, 0.0), r, np.nextafter(r, 1.0))]
        assert (below, at, above) == (0.0, 0.0, 1.0)
        in_float = [R.filter_grids(case.tracking, case.static, p, 1, 1, False)[cell[a, b]]
                    for p in (np.nextafter(r, 0.0), r, np.nextafter(r, 1.0))]
        assert in_float == [0.0, 0.0, 0.0]


def test_outlier_threshold_cells():
    """filled = t - 1 is no evidence: alone it leaves the cell unknown, beside free > 0 the cell is free whatever the
    threshold on the ratio; filled = t and t + 1 count."""
    (case,) = C.outlier()
    for percent, t, cameras in case.options:
        if cameras != 1:
            continue
        for in_double in (False, True):
            got = R.filter_grids(case.tracking, case.static, percent, t, cameras, in_double)
            assert got[C.outlier_cell(0, t - 1)] == 0.5 and case.static[C.outlier_cell(0, t - 1)] == 0.5
            assert got[C.outlier_cell(5, t - 1)] == 0.0
            assert got[C.outlier_cell(0, t)] == 1.0 and got[C.outlier_cell(0, t + 1)] == 1.0
            assert got[C.outlier_cell(5, t)] == (0.0 if 5 / (5 + t) >= percent else 1.0)
    assert {t for _, t, _ in case.options} == set(C.OUTLIER_THRESHOLDS)


def test_camera_rule_cells():
    """k cameras seeing free make the cell free exactly when k >= num_cameras_seen_free (never, when that is more than
    there are cameras); one camera seeing filled wins over all the others seeing free."""
    cases = C.camera()
    assert [c.tracking.shape[0] for c in cases] == C.CAMERA_GRIDS
    for case in cases:
        grids = case.tracking.shape[0]
        assert {n for _, _, n in case.options} == {1, grids, grids + 1}
        for (percent, outlier, cameras), in_double in _runs(case):
            got = R.filter_grids(case.tracking, case.static, percent, outlier, cameras, in_double)
            for k in range(grids + 1):
                for first in range(grids):
                    assert got[C.camera_free_cell(grids, k, first)] == (0.0 if k >= cameras else 0.5)
            for filled_camera in range(grids):
                cell = C.camera_filled_cell(grids, filled_camera)
                assert (case.tracking[:, cell, 1] > 0).sum() == 1 and (case.tracking[:, cell, 0] > 0).sum() == grids - 1
                assert got[cell] == 1.0


def test_static_occupancy_row():
    values = C.static_values()
    want = [np.nextafter(np.float32(0.5), np.float32(1)), np.float32(0.5), np.nextafter(np.float32(0.5), np.float32(0)),
            np.float32(-0.0), np.float32(1e-45), np.float32(-1), np.float32(-np.inf), np.float32(0.0), np.float32(0.75),
            np.float32(2), np.float32(np.inf), np.float32(1)]
    assert bits_equal(values[:len(want)], np.array(want, dtype=np.float32))
    assert np.isnan(values[len(want):]).all() and len(values) == len(want) + 4
    (case,) = C.static()
    assert np.array_equal(R.skipped(case.static), C.static_skipped())
    with np.errstate(invalid="ignore"):
        greater = case.static > np.float32(0.5)
    assert (C.static_skipped() & ~greater).sum() == 4 * len(C.STATIC_PATTERNS)    # the NaN cells: skipped, yet not > 0.5
    for (percent, outlier, cameras), in_double in _runs(case):
        got = R.filter_grids(case.tracking, case.static, percent, outlier, cameras, in_double)
        assert bits_equal(got[C.static_skipped()], case.static[C.static_skipped()])
        # a cell at or below 0.5 forgets its static value: -0.0, -1 and -inf give what 0.5 gives
        per_value = got.reshape(len(values), len(C.STATIC_PATTERNS))
        for row in np.flatnonzero(~np.array([s for _, s in C.STATIC_BITS])):
            assert bits_equal(per_value[row], per_value[1])


@pytest.mark.parametrize("counts", C.SPLIT_GRIDS)
def test_split_scenes_reach_the_ends_of_the_accumulation(counts):
    """What the share-accumulation tests rely on: the cloud's last quarter -- part of a helper's share under every
    split -- counts in the grid's last cell (the scalar tail, where the cell count is odd), and on the large grid beyond
    the accumulate kernel's launch cap and in its last four ints."""
    scene = C.split_scene(counts)
    before, whole, again, last_quarter = C.split_expected(counts)
    ints = 2 * int(np.prod(counts))
    assert len(scene.points) >= 8 and before.min() >= 1
    assert last_quarter.reshape(-1)[-2:].any() and again.reshape(-1)[-2:].any()
    assert whole.sum() > last_quarter.sum() > 0
    if counts == (162, 162, 162):
        assert ints > C.ACCUMULATE_CAP_INTS and 161 ** 3 * 2 <= C.ACCUMULATE_CAP_INTS
        assert last_quarter.reshape(-1)[C.ACCUMULATE_CAP_INTS:].any() and last_quarter.reshape(-1)[-4:].any()
        assert np.count_nonzero(whole.reshape(-1)[C.ACCUMULATE_CAP_INTS:]) > 100
        assert np.count_nonzero(whole.reshape(-1)[:C.ACCUMULATE_CAP_INTS]) > 100
    else:
        assert ints <= C.ACCUMULATE_CAP_INTS
    assert [2 * int(np.prod(c)) % 4 for c in C.SPLIT_GRIDS] == [2, 2, 2, 2, 0]
