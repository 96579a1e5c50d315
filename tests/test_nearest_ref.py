"""(not gpu) The checker of the nearest-other-class tests (tests/nearest_ref.py): its brute-force reference equals
oracle.edt3d on seeded random grids, it accepts correct answers -- whichever of the tied cells they name -- and
rejects each kind of wrong one."""
import numpy as np
import pytest

import nearest_ref as R


def _correct(filled):
    """A correct (nearest, d2) by brute force, taking the LAST of the tied candidates (so not any kernel's choice)."""
    filled = np.asarray(filled, dtype=bool)
    coords = np.stack(np.unravel_index(np.arange(filled.size), filled.shape), axis=1).astype(np.int64)
    flat = filled.ravel()
    nearest = np.full(filled.size, R.NO_INDEX, dtype=np.int32)
    d2 = np.full(filled.size, R.NO_DISTANCE, dtype=np.int32)
    for c in range(filled.size):
        sites = np.flatnonzero(flat != flat[c])
        if sites.size:
            d = ((coords[sites] - coords[c]) ** 2).sum(axis=1)
            best = np.flatnonzero(d == d.min())[-1]
            nearest[c], d2[c] = sites[best], d[best]
    return nearest.reshape(filled.shape), d2.reshape(filled.shape)


@pytest.fixture(scope="module")
def scene():
    rng = np.random.RandomState(11)
    filled = rng.random_sample((6, 5, 7)) < 0.2
    filled[0, 0, 0], filled[5, 4, 6] = True, False
    nearest, d2 = _correct(filled)
    return filled, nearest, d2


@pytest.mark.parametrize("shape,fill,seed", [((7, 6, 5), 0.5, 1), ((12, 9, 14), 0.05, 2), ((1, 1, 17), 0.3, 3),
                                             ((20, 20, 20), 0.01, 4), ((5, 1, 9), 0.95, 5), ((4, 4, 4), 0.0, 6),
                                             ((3, 4, 2), 1.0, 7)])
def test_brute_force_equals_the_oracle(shape, fill, seed):
    filled = np.random.RandomState(seed).random_sample(shape) < fill
    want = R.reference_d2(filled)
    got = R.brute_force_d2(filled, chunk=37)
    assert np.array_equal(got, want)
    assert np.isinf(want).all() == (filled.all() or not filled.any())


def test_accepts_correct_answers_whatever_the_tie(scene):
    filled, nearest, d2 = scene
    R.check(filled, nearest)
    R.check(filled, nearest, d2)
    R.check(filled, nearest, d2, reference=R.brute_force_d2(filled))
    # the checkerboard: every cell ties; both of these name a neighbour
    board = np.indices((3, 3, 3)).sum(axis=0) % 2 == 1
    first, d2_first = _correct(board)
    R.check(board, first, d2_first)
    flat = board.ravel()
    coords = np.stack(np.unravel_index(np.arange(27), (3, 3, 3)), axis=1)
    other = np.array([[s for s in range(27) if flat[s] != flat[c] and ((coords[s] - coords[c]) ** 2).sum() == 1][0]
                      for c in range(27)], dtype=np.int32).reshape(3, 3, 3)
    assert not np.array_equal(other, first)
    R.check(board, other, d2_first)
    # grids of one class: -1 everywhere
    for value in (False, True):
        one = np.full((2, 3, 2), value)
        R.check(one, np.full(one.shape, -1, np.int32), np.full(one.shape, R.NO_DISTANCE, np.int32))


def _pick(filled, nearest, condition):
    for c in range(filled.size):
        if condition(c):
            return c
    raise AssertionError("the scene has no such cell")


def test_rejects_each_kind_of_wrong_answer(scene):
    filled, nearest, d2 = scene
    flat = filled.ravel()
    n = filled.size

    def broken(cell, value, field=nearest):
        out = field.copy()
        out.ravel()[cell] = value
        return out

    # a same-class target: the cell itself
    with pytest.raises(AssertionError, match="own class"):
        R.check(filled, broken(3, 3))
    # an off-by-one target: the next index is the cell's own class or farther away (a tie would be a correct answer)
    coords = np.stack(np.unravel_index(np.arange(n), filled.shape), axis=1).astype(np.int64)

    def next_index_is_wrong(c):
        t = nearest.ravel()[c] + 1
        return t < n and (flat[t] == flat[c] or ((coords[t] - coords[c]) ** 2).sum() != d2.ravel()[c])

    cell = _pick(filled, nearest, next_index_is_wrong)
    with pytest.raises(AssertionError, match="own class|the minimum is"):
        R.check(filled, broken(cell, nearest.ravel()[cell] + 1))
    # -1 where a target exists
    with pytest.raises(AssertionError, match="nearest -1"):
        R.check(filled, broken(5, -1))
    # a target where none exists
    one = np.zeros((2, 2, 2), dtype=bool)
    answer = np.full(one.shape, -1, np.int32)
    answer[1, 0, 1] = 0
    with pytest.raises(AssertionError, match="reference d2 inf"):
        R.check(one, answer)
    # a target outside the grid
    with pytest.raises(AssertionError, match="outside the grid"):
        R.check(filled, broken(7, n))
    with pytest.raises(AssertionError):
        R.check(filled, broken(7, -2))
    # a non-minimal target: the farthest cell of the other class
    cell = _pick(filled, nearest, lambda c: not flat[c])
    sites = np.flatnonzero(flat != flat[cell])
    far = sites[np.argmax(((coords[sites] - coords[cell]) ** 2).sum(axis=1))]
    assert far != nearest.ravel()[cell]
    with pytest.raises(AssertionError, match="the minimum is"):
        R.check(filled, broken(cell, far))
    # a wrong d2, and d2 without the "none" code
    with pytest.raises(AssertionError, match="d2"):
        R.check(filled, nearest, broken(9, d2.ravel()[9] + 1, d2))
    with pytest.raises(AssertionError, match="d2"):
        R.check(one, np.full(one.shape, -1, np.int32), np.zeros(one.shape, np.int32))
    # the dtype
    with pytest.raises(AssertionError, match="int32"):
        R.check(filled, nearest.astype(np.int64))
    with pytest.raises(AssertionError, match="int32"):
        R.check(filled, nearest, d2.astype(np.int64))
