"""(not gpu) tests/surface_ref.py against itself, against answers derived by hand and against the invariants of a closed
surface.  The GPU tests compare the device with this restatement bit for bit, so what is pinned here is pinned there."""
import numpy as np
import pytest

import surface_cases as C
import surface_ref as R


def _same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


@pytest.mark.parametrize("kind", C.FIELDS)
def test_loop_and_vectorised_forms_agree(kind):
    wfg = C.rotation_and_translation()
    seen = 0
    for shape in C.FLAT_SHAPES + C.SHAPES:
        values, iso, above = C.field(kind, shape)
        for transform in (None, wfg):
            want = R.extract_loop(values, 0.25, iso, above, transform)
            assert _same(R.extract(values, 0.25, iso, above, transform), want), (shape, transform is not None)
        if min(shape) == 1:
            assert len(want[0]) == 0 and len(want[1]) == 0
        seen += len(want[0])
    assert seen > 100


def test_the_fields_exercise_what_they_are_for():
    shape = (17, 9, 70)
    vertices, triangles, _ = R.extract(*_args("noise", shape))
    assert len(vertices) > 0.9 * 16 * 8 * 69
    values, iso, _ = C.field("equal", shape)
    assert (values == iso).sum() > 1000
    values, _, _ = C.field("nonfinite", shape)
    assert np.isnan(values).any() and np.isposinf(values).any() and np.isneginf(values).any()
    clean = np.where(np.isfinite(values), values, np.float32(0.5))
    assert len(R.extract(values, 1.0)[0]) < len(R.extract(clean, 1.0)[0])  # void cubes
    _, triangles, _ = R.extract(*_args("open", shape))
    assert len(triangles) and not R.is_closed(R.quads_of(triangles))
    _, triangles, _ = R.extract(*_args("blob", shape))
    assert len(triangles) and R.is_closed_manifold(R.quads_of(triangles))


def _args(kind, shape, resolution=1.0):
    values, iso, above = C.field(kind, shape)
    return values, resolution, iso, above


def test_one_inside_corner_of_a_single_cube():
    values = np.ones((2, 2, 2), dtype=np.float32)
    values[1, 0, 1] = -3.0
    for extract in (R.extract_loop, R.extract):
        vertices, triangles, cells = extract(values, 2.0)
        assert vertices.shape == (1, 3) and triangles.shape == (0, 3) and cells.tolist() == [0]
        # the three edges at (1, 0, 1): t = 1/4 from the outside end on x, 3/4 towards the corner ... by hand:
        # x edge (dy, dz) = (0, 1): v0 = 1, v1 = -3: t = (0 - 1) / (-3 - 1) = 0.25 -> (0.25, 0, 1)
        # y edge (dz, dx) = (1, 1): v0 = -3, v1 = 1: t = 3 / 4                  -> (1, 0.75, 1)
        # z edge (dx, dy) = (1, 0): v0 = 1, v1 = -3: t = 0.25                    -> (1, 0, 0.25)
        want = [((0.5 + (0.25 + 1.0 + 1.0) / 3.0) * 2.0), ((0.5 + (0.0 + 0.75 + 0.0) / 3.0) * 2.0),
                ((0.5 + (1.0 + 1.0 + 0.25) / 3.0) * 2.0)]
        assert vertices[0].tolist() == want


def test_one_inside_sample_in_a_3x3x3_field():
    values = np.ones((3, 3, 3), dtype=np.float32)
    values[1, 1, 1] = -1.0
    for extract in (R.extract_loop, R.extract):
        vertices, triangles, cells = extract(values, 1.0)
        assert vertices.shape == (8, 3) and triangles.shape == (12, 3)
        assert cells.tolist() == [(i * 3 + j) * 3 + k for i in (0, 1) for j in (0, 1) for k in (0, 1)]
        assert vertices[0].tolist() == [0.5 + 2.5 / 3] * 3          # cube (0, 0, 0): offset 5/6 on every axis
        assert vertices[7].tolist() == [1.5 + 0.5 / 3] * 3          # cube (1, 1, 1): offset 1/6
        # every normal points away from the inside sample at (1.5, 1.5, 1.5)
        for a, b, c in triangles:
            normal = np.cross(vertices[b] - vertices[a], vertices[c] - vertices[a])
            assert np.dot(normal, (vertices[a] + vertices[b] + vertices[c]) / 3 - 1.5) > 0
        quads = R.quads_of(triangles)
        assert R.is_closed_manifold(quads) and R.euler_characteristic(8, quads) == 2
        assert R.signed_volume(vertices, triangles) > 0
        # the first quad belongs to the x edge from p = (0, 1, 1), outside: (c00, c01, c11, c10) of the cubes
        # (0,0,0), (0,0,1), (0,1,1), (0,1,0) = vertices 0, 1, 3, 2
        assert triangles[0].tolist() == [0, 1, 3] and triangles[1].tolist() == [0, 3, 2]


@pytest.mark.parametrize("kind", sorted(C.SOLIDS))
def test_invariants_of_closed_surfaces(kind):
    filled = C.solid(kind)
    resolution = 0.25
    vertices, triangles, _ = R.extract(C.signed_edt(filled), resolution)
    quads = R.quads_of(triangles)
    assert R.is_closed_manifold(quads)
    assert R.euler_characteristic(len(vertices), quads) == C.SOLIDS[kind]
    volume = R.signed_volume(vertices, triangles)
    assert volume > 0
    # both surfaces lie inside the union of the active cubes (one vertex each)
    print(kind, "volume error in cells", abs(volume / resolution ** 3 - filled.sum()), "active cubes", len(vertices))
    assert abs(volume - filled.sum() * resolution ** 3) <= len(vertices) * resolution ** 3


def test_salt_is_closed_though_not_manifold():
    vertices, triangles, _ = R.extract(C.signed_edt(C.salt()), 1.0)
    quads = R.quads_of(triangles)
    assert len(quads) > 500
    assert R.is_closed(quads) and not R.is_closed_manifold(quads)
