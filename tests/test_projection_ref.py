"""(not gpu) tests/projection_ref.py, the CPU restatement of ProjectLocationOutOfCollisionToMinimumDistance that the
device is compared against (tests/test_gpu_projection.py), pinned by properties that do not depend on it."""
import numpy as np
import pytest

import projection_cases as C
import projection_ref as P


@pytest.fixture(scope="module")
def oracle():
    from oracle import oracle as O
    return O


def same_doubles(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


CASES = [("spheres", 0.0, 0), ("spheres", 1.5, 0), ("dense", 0.0, 0), ("corridor", 3.0, 0), ("corridor", 3.0, 7),
         ("corridor", 0.0, 0), ("flat_1x6x5", 0.0, 0), ("tiny_2x2x2", 0.0, 0)]


@pytest.mark.parametrize("name,clearance_cells,max_iterations", CASES)
def test_properties_of_the_restatement(oracle, name, clearance_cells, max_iterations):
    sdf, res = C.scene(name)
    q = C.queries(name)
    minimum_distance = clearance_cells * res
    multiplier = 0.1
    pos, has, status, iterations = P.project_out_of_collision(oracle, sdf, res, q, minimum_distance, multiplier,
                                                              max_iterations)
    limit = max_iterations or P.default_max_iterations(sdf.shape, multiplier)
    start_d, start_in = oracle.estimate_distance(sdf, res, q)
    ok, outside = status == P.OK, status == P.OUTSIDE
    assert np.array_equal(has, ok | outside)
    # OUTSIDE: exactly the starts that are not in the grid (NaN and infinite ones too), bit-unchanged
    assert np.array_equal(outside, ~start_in)
    assert same_doubles(pos[outside], q[outside])
    # OK: clear of the minimum distance; without a step, bit-unchanged; never further than the steps allow
    end_d, end_in = oracle.estimate_distance(sdf, res, pos[ok])
    assert end_in.all() and (end_d > minimum_distance).all()
    unmoved = ok & (iterations == 0)
    assert same_doubles(pos[unmoved], q[unmoved])
    assert np.array_equal(unmoved, ok & (start_d > minimum_distance))
    moved = np.sqrt(((pos[ok] - q[ok]) ** 2).sum(axis=1))
    assert (moved <= iterations[ok] * (res * multiplier) * (1 + 1e-12)).all()
    # no value: NaN x3; the limit is reached by those that report it and exceeded by none
    assert np.isnan(pos[~has]).all()
    assert (iterations[status == P.ITERATION_LIMIT] == limit).all()
    assert (iterations <= limit).all() and (iterations[outside] == 0).all()
    assert (iterations[status == P.LEFT_GRID] >= 1).all()


def test_statuses_that_the_cases_are_there_for(oracle):
    sdf, res = C.scene("spheres")
    _, _, status, _ = P.project_out_of_collision(oracle, sdf, res, C.queries("spheres"), 1.5 * res)
    assert set(np.unique(status)) == {P.OK, P.OUTSIDE, P.FLAT_GRADIENT, P.LEFT_GRID, P.ITERATION_LIMIT}
    sdf, res = C.scene("corridor")
    for max_iterations in (0, 7):                            # the gradients of the two walls point at each other
        _, _, status, iterations = P.project_out_of_collision(oracle, sdf, res, C.queries("corridor"), 0.3, 0.1,
                                                              max_iterations)
        assert (status == P.ITERATION_LIMIT).all() and (iterations == (max_iterations or 520)).all()
    _, _, status, iterations = P.project_out_of_collision(oracle, sdf, res, C.queries("corridor"), 0.0)
    assert (status == P.OK).all() and iterations.max() <= 15


def test_one_filled_voxel_by_hand(oracle):
    """5^3 cells of 0.1 with the centre voxel filled: its field is -0.1 there and +0.1 in the six face neighbours.  At
    the centre of the filled voxel the estimate is -0.1 + 0.05 <= 0 and the central differences are 0 on every axis: no
    result.  At the centre of a face neighbour the estimate is +0.1 - 0.05 > 0: returned as it is, no step."""
    sdf, res = C.scene("one_voxel")
    assert sdf[2, 2, 2] == np.float32(-0.1) and sdf[3, 2, 2] == np.float32(0.1)
    centre = (np.array([2.0, 2.0, 2.0]) + 0.5) * res
    neighbour = (np.array([3.0, 2.0, 2.0]) + 0.5) * res
    off_centre = centre + np.array([0.02, 0.0, 0.0])
    q = np.stack([centre, neighbour, off_centre])
    pos, has, status, iterations = P.project_out_of_collision(oracle, sdf, res, q)
    assert status.tolist() == [P.FLAT_GRADIENT, P.OK, P.FLAT_GRADIENT]   # (the whole cell has the centre's gradient)
    assert has.tolist() == [False, True, False] and iterations.tolist() == [0, 0, 0]
    assert np.isnan(pos[0]).all() and same_doubles(pos[1], neighbour)


def test_frames(oracle):
    """The same walk seen from a rotated and translated frame gives the grid-frame results moved into that frame.  Starts
    that lie exactly on a cell boundary are left out: there the rounding of the frame change decides the cell."""
    sdf, res = C.scene("spheres")
    q = C.queries("spheres")
    interior = np.ones(len(q), dtype=bool)
    interior[::17] = False
    q = q[interior & np.isfinite(q).all(axis=1)]
    grid_from_world, rotation, world_from_grid = C.frame_pair()
    pos, has, status, iterations = P.project_out_of_collision(oracle, sdf, res, q)
    wpos, whas, wstatus, witerations = P.project_out_of_collision(oracle, sdf, res, C.to_world(q, world_from_grid), 0.0,
                                                                  0.1, 0, grid_from_world, rotation)
    assert np.array_equal(status, wstatus) and np.array_equal(iterations, witerations)
    assert len(np.unique(status)) >= 3 and iterations.max() > 20
    assert np.abs(C.to_world(pos[has], world_from_grid) - wpos[has]).max() < 1e-9
