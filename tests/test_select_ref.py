"""(not gpu) tests/select_ref.py against itself and against hand-derived answers: the literal IsSurfaceIndex loop and
the vectorised form agree on every shared case, and the rules give what a reader of the reference would expect."""
import numpy as np

import select_cases as C
import select_ref as R


def test_literal_and_vectorised_26_rule_agree():
    for shape in C.SMALL_SHAPES + [(6, 5, 7)]:
        for name, (values, _) in C.value_sets(shape, seed=sum(shape)).items():
            assert np.array_equal(R.surface26_literal(values), R.surface26(values)), (shape, name)


def test_centre_cell_makes_all_27_surface():
    occ = np.zeros((3, 3, 3), np.float32)
    occ[1, 1, 1] = 1.0
    assert R.surface26_literal(occ).all() and R.surface26(occ).all()
    assert len(R.select(occ, R.SELECT_SURFACE_26, 15)[0]) == 27
    assert list(R.select(occ, R.SELECT_SURFACE_26, R.CLASS_ABOVE)[0]) == [13]


def test_core_centre_is_not_surface():
    occ = np.zeros((5, 5, 5), np.float32)
    occ[1:4, 1:4, 1:4] = 1.0
    got = R.surface26_literal(occ)
    assert not got[2, 2, 2]
    assert got[1:4, 1:4, 1:4].sum() == 26 and got.sum() == 125 - 1      # every free cell touches the core
    assert np.array_equal(got, R.surface26(occ))


def test_uniform_grid():
    occ = np.full((4, 5, 6), 1.0, np.float32)
    assert not R.surface26_literal(occ).any() and not R.surface26(occ).any()
    labels = np.ones(occ.shape, np.uint32)
    faces = R.component_surface(labels)
    assert faces.sum() == 4 * 5 * 6 - 2 * 3 * 4 and not faces[1:-1, 1:-1, 1:-1].any()


def test_single_nan_in_a_free_grid():
    occ = np.zeros((5, 5, 5), np.float32)
    occ[2, 2, 2] = np.nan
    for got in (R.surface26_literal(occ), R.surface26(occ)):
        assert not got.any()                                               # NaN >= 0.5 is false


def test_single_nan_in_a_grid_of_one_half():
    occ = np.full((5, 5, 5), 0.5, np.float32)
    occ[2, 2, 2] = np.nan
    for got in (R.surface26_literal(occ), R.surface26(occ)):
        assert not got[2, 2, 2]
        want = np.zeros(occ.shape, bool)
        want[1:4, 1:4, 1:4] = True
        want[2, 2, 2] = False
        assert np.array_equal(got, want)                                   # NaN != 0.5 is true


def test_classes_and_order():
    values = np.array([[[0.0, 0.5, 1.0, np.nan, np.inf, -np.inf]]], np.float32)
    assert list(R.classes(values, 0.5).reshape(-1)) == [2, 4, 1, 8, 1, 2]
    assert list(R.classes(np.array([-0.0, 0.0, np.nan], np.float32), 0.0)) == [4, 4, 8]
    indices, vals, labels = R.select(values, R.SELECT_ALL, R.CLASS_ABOVE | R.CLASS_UNORDERED,
                                     labels=np.arange(6, dtype=np.uint32).reshape(1, 1, 6))
    assert indices.dtype == np.int32 and list(indices) == [2, 3, 4] and list(labels) == [2, 3, 4]
    assert vals[0] == 1.0 and np.isnan(vals[1]) and vals[2] == np.inf


def test_component_surface_matches_the_dense_mask_reference():
    import components_ref
    for shape in C.SMALL_SHAPES:
        values, labels = C.value_sets(shape, seed=3)["random"]
        for types in range(1, 8):
            mask = types & 3 | (12 if types & 4 else 0)                     # "unknown" is equal | unordered
            want = np.flatnonzero(components_ref.surface_mask(values, labels, types).reshape(-1))
            assert np.array_equal(R.select(values, R.SELECT_COMPONENT_SURFACE, mask, labels=labels)[0], want)


def test_value_sets_select_nothing_and_everything():
    for shape in C.SMALL_SHAPES[1:]:
        sets = C.value_sets(shape)
        n = int(np.prod(shape))
        for rule in (R.SELECT_ALL, R.SELECT_SURFACE_26, R.SELECT_COMPONENT_SURFACE):
            values, labels = sets["everything"]
            assert len(R.select(values, rule, 15, labels=labels)[0]) == n, (shape, rule)
        values, labels = sets["uniform"]
        assert len(R.select(values, R.SELECT_SURFACE_26, 15)[0]) == 0
        assert len(R.select(values, R.SELECT_ALL, 13)[0]) == 0
