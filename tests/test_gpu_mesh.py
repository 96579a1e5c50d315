"""(gpu) The mesh rasterizer on the device against the CPU restatement of tests/mesh_ref.py: every comparison is
np.array_equal on the whole map -- every voxel, no tolerance, no exclusions."""
import numpy as np
import pytest

import mesh_ref as M
from conftest import bits_equal
from oracle import oracle as O
from test_mesh_ref import ONE, SHIFTS, SLANTED, independent_meshes
from voxelized_geometry_tools_amd import capi, synthetic

pytestmark = pytest.mark.gpu

RULES = (capi.MESH_RULE_REFERENCE, capi.MESH_RULE_NEAREST)
CELL = capi.OCCUPANCY_COMPONENT_CELL
MARK = 0xABCD0123


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def _translation(origin):
    origin = np.asarray(origin, np.float64)
    return synthetic.translation_xform(*origin), synthetic.translation_xform(*(-origin))


def _meshes():
    """(name, vertices, triangles, resolution): small meshes of every generator."""
    v, t = synthetic.mesh_box((0.11, -0.2, 0.3), (0.93, 0.41, 0.77))
    yield "box", v, t, 0.04
    v, t = synthetic.mesh_torus(0.5, 0.17, 24, 12, (0.3, 0.2, 0.1))
    yield "torus", v, t, 0.03
    yield "slanted", SLANTED, ONE, 0.125
    for name, v, t, res in independent_meshes():
        yield name, v, t, res


def _check_map(ctx, vertices, triangles, shape, res, wfg, gfw, rule, before=None, enforce=False):
    """Host form with 4-byte and 8-byte cells against the restatement; returns the expected map."""
    before = np.zeros(shape, np.float32) if before is None else before
    want = M.rasterize(vertices, triangles, before, res, wfg, gfw, enforce, rule)
    got = ctx.rasterize_mesh(vertices, triangles, before.copy(), res, wfg, gfw, enforce, rule)
    assert got.dtype == np.float32 and np.array_equal(got, want)
    rec = np.zeros(shape, dtype=CELL)
    rec["occupancy"] = before
    rec["component"] = MARK
    ctx.rasterize_mesh(vertices, triangles, rec, res, wfg, gfw, enforce, rule)
    assert np.array_equal(rec["occupancy"], want) and (rec["component"] == MARK).all()   # the other 4 bytes: untouched
    return want


@pytest.mark.parametrize("rule", RULES)
def test_new_maps_of_every_generator(ctx, rule):
    """The map RasterizeMeshIntoOccupancyMap builds (a translated grid, enforce on), both cell sizes."""
    for name, v, t, res in _meshes():
        shape, origin = capi.mesh_grid_for(v, res)
        wfg, gfw = _translation(origin)
        want = _check_map(ctx, v, t, shape, res, wfg, gfw, rule, enforce=True)
        assert want.any() and np.array_equal(want, M.rasterize_into_new_map(v, t, res, rule)[0]), name


def test_known_answer_of_the_reference_test(ctx):
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    shape, origin = capi.mesh_grid_for(v, 0.125)
    assert shape == (10, 10, 2)
    got = ctx.rasterize_mesh(v, ONE, np.zeros(shape, np.float32), 0.125, *_translation(origin), True, 0)
    x, y = np.meshgrid(np.arange(10), np.arange(10), indexing="ij")
    assert not got[:, :, 0].any() and np.array_equal(got[:, :, 1], ((x >= 1) & (y >= 1) & (y < 10 - x)).astype(np.float32))


@pytest.mark.parametrize("rule", RULES)
def test_rule_fixture_and_its_translations(ctx, rule):
    maps = []
    for shift in SHIFTS:
        v = SLANTED + np.array(shift)
        shape, origin = capi.mesh_grid_for(v, 0.125)
        maps.append(_check_map(ctx, v, ONE, shape, 0.125, *_translation(origin), rule, enforce=True))
    same = [np.array_equal(maps[0], m) for m in maps[1:]]
    assert same == ([False, False] if rule == 0 else [True, True])


@pytest.mark.parametrize("rule", RULES)
def test_identity_translated_and_rotated_transforms(ctx, rule):
    v, t = synthetic.mesh_icosphere(2, 0.41, (0.6, 0.55, 0.5))
    shape, res = (30, 29, 27), 0.04
    _check_map(ctx, v, t, shape, res, None, None, rule)                                  # the grid frame
    identity = synthetic.translation_xform(0.0, 0.0, 0.0)
    _check_map(ctx, v, t, shape, res, identity, identity, rule)
    wfg, gfw = synthetic.rigid_xform((0.0, 0.0, 1.0), 0.0, (-0.07, 0.013, 0.1))
    _check_map(ctx, v, t, shape, res, wfg, gfw, rule)
    wfg, gfw = synthetic.rigid_xform((1.0, -2.0, 0.5), 0.6, (0.2, -0.3, 0.1))
    world = synthetic.mesh_transformed(v, wfg)                                           # the mesh moves with the grid
    want = _check_map(ctx, world, t, shape, res, wfg, gfw, rule)
    assert want.sum() > 500
    # and a grid rotated against the mesh: ranges from a rotated box, some of them empty or clipped
    _check_map(ctx, v, t, shape, res, wfg, gfw, rule)


@pytest.mark.parametrize("rule", RULES)
def test_device_pointers(ctx, rule):
    import torch
    for name, v, t, res in _meshes():
        shape, origin = capi.mesh_grid_for(v, res)
        wfg, gfw = _translation(origin)
        want = M.rasterize(v, t, np.zeros(shape, np.float32), res, wfg, gfw, True, rule)
        v_dev = torch.from_numpy(np.ascontiguousarray(v, np.float64)).cuda()
        t_dev = torch.from_numpy(np.ascontiguousarray(t, np.int32)).cuda()
        for enforce in (True, False):
            occ_dev = torch.zeros(shape, dtype=torch.float32, device="cuda")
            rec_dev = torch.full(shape + (2,), 7, dtype=torch.int32, device="cuda")       # 8-byte cells
            rec_dev[..., 0] = 0
            torch.cuda.synchronize()
            ctx.rasterize_mesh_dev(v_dev.data_ptr(), len(v), t_dev.data_ptr(), len(t), occ_dev.data_ptr(), 4, shape,
                                   res, wfg, gfw, enforce, rule)
            ctx.rasterize_mesh_dev(v_dev.data_ptr(), len(v), t_dev.data_ptr(), len(t), rec_dev.data_ptr(), 8, shape,
                                   res, wfg, gfw, enforce, rule)
            ctx.synchronize()
            assert np.array_equal(occ_dev.cpu().numpy(), want), (name, enforce)
            rec = rec_dev.cpu().numpy()
            assert np.array_equal(rec[..., 0].view(np.float32), want) and (rec[..., 1] == 7).all(), (name, enforce)


def test_a_map_that_already_holds_occupancy(ctx):
    v, t = synthetic.mesh_torus(0.5, 0.17, 24, 12, (0.8, 0.8, 0.3))
    shape, res = (40, 41, 15), 0.04
    rng = np.random.default_rng(3)
    before = rng.choice(np.array([0.0, 0.25, 0.5, 0.75, 1.0], np.float32), size=shape)
    for rule in RULES:
        want = _check_map(ctx, v, t, shape, res, None, None, rule, before=before)
        changed = want != before
        assert changed.any() and (want[changed] == 1.0).all()


def test_extents_off_the_wave_size_and_a_single_layer(ctx):
    res = 0.02
    v, t = synthetic.mesh_icosphere(2, 0.6, (0.7, 0.35, 1.0))
    for rule in RULES:
        assert _check_map(ctx, v, t, (70, 35, 100), res, None, None, rule).any()         # nz = 100: 64 + 36
        assert _check_map(ctx, v, t, (65, 33, 131), res, None, None, rule).any()
    v, t = synthetic.mesh_icosphere(2, 0.4, (0.5, 0.5, 0.013))
    for rule in RULES:
        assert _check_map(ctx, v, t, (50, 50, 1), res, None, None, rule).any()           # nz = 1: a slice of the sphere


def test_one_triangle_larger_than_the_grid(ctx):
    v = np.array([[-50.0, -40.0, 0.31], [60.0, -45.0, 0.29], [3.0, 70.0, 0.42]])
    for rule in RULES:
        want = _check_map(ctx, v, ONE, (24, 20, 70), 0.01, None, None, rule, enforce=False)
        assert want.sum() >= 24 * 20


def test_enforce_error_and_message(ctx):
    v, t = synthetic.mesh_icosphere(1, 0.3, (0.25, 0.25, 0.25))
    occ = np.full((10, 10, 10), 0.5, np.float32)
    with pytest.raises(capi.VgtHipError, match=r"Triangle is not contained by occupancy map \(triangle \d+\)"):
        ctx.rasterize_mesh(v, t, occ, 0.05, None, None, True, 0)
    assert (occ == 0.5).all()                                                            # the host map is not written
    with pytest.raises(RuntimeError, match=M.NOT_CONTAINED):
        M.rasterize(v, t, occ, 0.05, None, None, True, 0)
    assert _check_map(ctx, v, t, (10, 10, 10), 0.05, None, None, 0, enforce=False).any()
    # far outside: the literal range is refused before any brick runs
    with pytest.raises(ValueError, match="2\\^36"):
        ctx.rasterize_mesh(v * 1.0e6, t, occ, 0.05, None, None, True, 0)
    assert (occ == 0.5).all()


def test_status_errors(ctx):
    v = np.array([[0.1, 0.1, 0.1], [0.3, 0.1, 0.1], [0.1, 0.3, 0.1], [0.2, 0.2, 0.3]])
    good = [[0, 1, 2], [0, 1, 3]]
    occ = np.zeros((8, 8, 8), np.float32)
    for bad in ([0, 1, 4], [0, -1, 2]):
        with pytest.raises(ValueError, match="triangle 2 has a vertex index out of range"):
            ctx.rasterize_mesh(v, good + [bad], occ, 0.05)
    nan = v.copy()
    nan[3, 1] = np.nan
    with pytest.raises(ValueError, match="triangle 1 has a non-finite vertex"):
        ctx.rasterize_mesh(nan, good, occ, 0.05)
    inf = v.copy()
    inf[2, 0] = np.inf
    with pytest.raises(ValueError, match="triangle 0 has a non-finite vertex"):
        ctx.rasterize_mesh(inf, good, occ, 0.05)
    for bad in ([0, 1, 1], [2, 2, 2]):
        with pytest.raises(ValueError, match="triangle 1 is degenerate"):
            ctx.rasterize_mesh(v, [good[0], bad], occ, 0.05)
    collinear = np.array([[0.1, 0.1, 0.1], [0.2, 0.2, 0.2], [0.4, 0.4, 0.4]])
    with pytest.raises(ValueError, match="triangle 0 is degenerate"):
        ctx.rasterize_mesh(collinear, ONE, occ, 0.05)
    assert not occ.any()
    assert ctx.rasterize_mesh(v, np.zeros((0, 3), np.int32), occ, 0.05) is occ and not occ.any()   # no triangles
    assert ctx.rasterize_mesh(v, good, occ, 0.05).any()                                  # the context still works


@pytest.mark.parametrize("rule", RULES)
def test_large_mesh_on_a_large_grid(ctx, rule):
    import torch
    v, t = synthetic.mesh_icosphere(5, 1.27, (0.013, -0.007, 0.021))
    res = 0.01
    assert len(t) >= 20000
    shape, origin = capi.mesh_grid_for(v, res)
    assert min(shape) >= 256
    wfg, gfw = _translation(origin)
    want = M.rasterize(v, t, np.zeros(shape, np.float32), res, wfg, gfw, True, rule)
    assert want.sum() > 100000
    v_dev = torch.from_numpy(v).cuda()
    t_dev = torch.from_numpy(t).cuda()
    occ_dev = torch.zeros(shape, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.rasterize_mesh_dev(v_dev.data_ptr(), len(v), t_dev.data_ptr(), len(t), occ_dev.data_ptr(), 4, shape, res, wfg,
                           gfw, True, rule)
    ctx.synchronize()
    assert np.array_equal(occ_dev.cpu().numpy(), want)
    del occ_dev
    assert np.array_equal(ctx.rasterize_mesh(v, t, np.zeros(shape, np.float32), res, wfg, gfw, False, rule), want)


@pytest.mark.parametrize("rule", RULES)
def test_mesh_sdf_equals_the_oracle_on_the_restatements_map(ctx, rule):
    for name, v, t, res in _meshes():
        occ, origin = M.rasterize_into_new_map(v, t, res, rule)
        want, wlo, whi = O.sdf_from_occupancy(occ, res)
        got, lo, hi, got_origin, got_occ = ctx.mesh_sdf(v, t, res, rule=rule, with_occupancy=True)
        assert np.array_equal(got_occ, occ) and np.array_equal(got_origin, origin), name
        assert bits_equal(got, want) and (lo, hi) == (wlo, whi), name
