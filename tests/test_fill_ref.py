"""(not gpu) The numpy restatement of vgt_hip_fill_enclosed (tests/fill_ref.py) pinned: against hand cases whose counts
are written out, against scipy.ndimage.binary_fill_holes where scipy imports, its routes to "outside" against each
other, and the number of cells the project's test meshes enclose under the two closest-point rules."""
import numpy as np
import pytest

import fill_ref as F
import mesh_ref as M
from voxelized_geometry_tools_amd import synthetic

ROUTES = (F.outside_by_labels, F.outside_by_growing, F.outside_quick)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _grids():
    for name, occ, uif, _ in F.hand_cases():
        yield name, occ, uif
    for sealed in (True, False):
        yield "snake", F.snake((9, 11, 20), sealed)[0], True
    for shape, p in (((17, 19, 33), 0.6), ((5, 9, 130), 0.6), ((24, 24, 24), 0.75)):
        for uif in (True, False):
            yield "random", F.random_pockets(shape, p, 11, sprinkle=True), uif
    yield "hollow_spheres", synthetic.hollow_spheres((48, 40, 56), seed=5), True


@pytest.mark.parametrize("name, occ, uif, count", F.hand_cases(), ids=[c[0] for c in F.hand_cases()])
def test_hand_cases(name, occ, uif, count):
    for route in ROUTES:
        got, n = F.fill(occ, uif, route)
        assert n == count, route.__name__
        changed = _bits(got) != _bits(occ)
        assert changed.sum() == count and (got[changed] == 1.0).all()          # nothing else changes, bit for bit
        assert F.fill(got, uif, route)[1] == 0                                  # idempotent


def test_values_that_are_not_written_keep_their_bits():
    case = {name: occ for name, occ, _, _ in F.hand_cases()}
    got, _ = F.fill(case["odd_values"])
    assert np.signbit(got[0, 0, 0]) and got[1, 1, 1] == np.float32(0.7) and (got[2:4, 2, 1:3] == 1.0).all()
    got, _ = F.fill(case["nan_in_a_corner"])
    assert np.isnan(got[0, 0, 0]) and got[1, 1, 1] == 1.0
    got, _ = F.fill(case["nan_in_the_cavity"])
    assert got[1, 1, 1] == 1.0


def test_the_routes_agree():
    for name, occ, uif in _grids():
        want = F.fill(occ, uif, ROUTES[0])
        for route in ROUTES[1:]:
            got = F.fill(occ, uif, route)
            assert got[1] == want[1] and np.array_equal(_bits(got[0]), _bits(want[0])), (name, route.__name__)


def test_degenerate_extents_and_uniform_grids():
    rng = np.random.default_rng(2)
    for shape in ((1, 33, 67), (20, 1, 65), (7, 9, 1), (1, 1, 1), (2, 2, 2), (2, 9, 9)):
        assert F.fill((rng.random(shape) < 0.6).astype(np.float32))[1] == 0
    assert F.fill(np.zeros((5, 6, 7), np.float32))[1] == 0 and F.fill(np.ones((5, 6, 7), np.float32))[1] == 0


def test_sealed_and_opened_snake():
    occ, corridor = F.snake((9, 11, 20))
    assert corridor > 300 and F.fill(occ)[1] == corridor
    assert F.fill(F.snake((9, 11, 20), sealed=False)[0])[1] == 0


def test_against_binary_fill_holes():
    ndimage = pytest.importorskip("scipy.ndimage")
    total = 0
    for name, occ, uif in _grids():
        filled = ~F.passable(occ, uif)
        want = ndimage.binary_fill_holes(filled)                               # (default structure: the six faces)
        got, count = F.fill(occ, uif)
        assert np.array_equal(~F.passable(got, uif), want), name
        assert count == int(want.sum()) - int(filled.sum()), name
        total += count
    assert total > 1000


def _mesh_cases():
    v, t = synthetic.mesh_torus(0.5, 0.17, 24, 12, (0.3, 0.2, 0.1))
    yield "torus_nearest", v, t, 0.03, 1, (47, 47, 14), 7070
    yield "torus_reference", v, t, 0.03, 0, (47, 47, 14), 1                     # the shell leaks along slanted edges
    v, t = synthetic.mesh_box((0.11, -0.2, 0.3), (0.93, 0.41, 0.77))
    for rule in (0, 1):
        yield "box", v, t, 0.04, rule, None, 3080
    for subdivisions, res, count in ((2, 0.05, 1472), (1, 0.08, 280)):
        v, t = synthetic.mesh_icosphere(subdivisions, 0.4, (0.0, 0.0, 0.0))
        for rule in (0, 1):
            yield "icosphere%d" % subdivisions, v, t, res, rule, None, count


@pytest.mark.parametrize("name, v, t, res, rule, shape, count", list(_mesh_cases()),
                         ids=["%s-%d" % (c[0], c[4]) for c in _mesh_cases()])
def test_cells_the_test_meshes_enclose(name, v, t, res, rule, shape, count):
    occ, _ = M.rasterize_into_new_map(v, t, res, rule)
    assert shape is None or occ.shape == shape
    assert F.fill(occ)[1] == count
