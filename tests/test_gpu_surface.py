"""(gpu) The surface extraction on the device against tests/surface_ref.py.  Every output is compared bit for bit:
the vertices as bytes, the triangles, the vertex cells and both counts."""
import ctypes
import functools

import numpy as np
import pytest

import surface_cases as C
import surface_ref as R
from voxelized_geometry_tools_amd import capi, synthetic

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A
ALL_SHAPES = C.FLAT_SHAPES + C.SHAPES
_ids = lambda s: "x".join(map(str, s))  # noqa: E731


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def _reference(kind, shape, resolution=0.25, transformed=False):
    """(values, iso, inside_above, (vertices, triangles, cells)): computed once, shared, never modified."""
    values, iso, above = C.field(kind, shape)
    want = R.extract(values, resolution, iso, above, C.rotation_and_translation() if transformed else None)
    for array in (values,) + want:
        array.setflags(write=False)
    return values, iso, above, want


def _same(got, want):
    got = [np.ascontiguousarray(g.cpu().numpy() if hasattr(g, "cpu") else g) for g in got]
    return len(got) == len(want) and all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes()
                                         for g, w in zip(got, want))


@pytest.mark.parametrize("kind", C.FIELDS)
def test_every_field_on_every_shape(ctx, kind):
    vertices = 0
    for shape in ALL_SHAPES:
        values, iso, above, want = _reference(kind, shape)
        got = ctx.extract_surface(values, 0.25, iso, above, with_cells=True)
        assert _same(got, want), shape
        if min(shape) == 1:
            assert len(got[0]) == 0 and len(got[1]) == 0
        vertices += len(got[0])
    assert vertices > 100


@pytest.mark.parametrize("kind", ["blob", "noise", "nonfinite"])
def test_transform_and_resolutions(ctx, kind):
    shape = (17, 9, 70)
    for resolution in (0.01, 0.25):
        for transformed in (False, True):
            values, iso, above, want = _reference(kind, shape, resolution, transformed)
            got = ctx.extract_surface(values, resolution, iso, above,
                                      C.rotation_and_translation() if transformed else None, with_cells=True)
            assert _same(got, want), (resolution, transformed)
    # vertices alone, and the pair without the cells
    values, iso, above, want = _reference(kind, shape)
    assert _same(ctx.extract_surface(values, 0.25, iso, above), want[:2])


class DeviceMesh:
    """A field on the device and sentinel-filled outputs with room for `spare` entries more than the mesh needs."""

    def __init__(self, torch, values, want, spare=5):
        self.values = torch.from_numpy(values.copy()).cuda()
        self.shape = values.shape
        self.nv, self.nt = len(want[0]), len(want[1])
        self.vertices = torch.full((self.nv + spare, 3), float(SENTINEL), dtype=torch.float64, device="cuda")
        self.cells = torch.full((self.nv + spare,), SENTINEL, dtype=torch.int32, device="cuda")
        self.triangles = torch.full((self.nt + spare, 3), SENTINEL, dtype=torch.int32, device="cuda")

    def untouched(self, first_vertex=0, first_triangle=0):
        return bool((self.vertices[first_vertex:] == float(SENTINEL)).all() and
                    (self.cells[first_vertex:] == SENTINEL).all() and
                    (self.triangles[first_triangle:] == SENTINEL).all())

    def run(self, ctx, iso, above, vertex_capacity, triangle_capacity, outputs=True, resolution=0.25):
        nv, nt = ctypes.c_int64(-1), ctypes.c_int64(-1)
        ptr = (lambda t: t.data_ptr()) if outputs else (lambda t: None)
        rc = ctx._lib.vgt_hip_extract_surface_dev(
            ctx.handle, self.values.data_ptr(), *self.shape, iso, int(above), resolution, None, ptr(self.vertices),
            ptr(self.cells), vertex_capacity, ptr(self.triangles), triangle_capacity, ctypes.byref(nv), ctypes.byref(nt))
        return rc, int(nv.value), int(nt.value)

    def mesh(self):
        return self.vertices[:self.nv], self.triangles[:self.nt], self.cells[:self.nv]


def test_capacities(ctx, torch):
    values, iso, above, want = _reference("blob", (17, 9, 70))
    mesh = DeviceMesh(torch, values, want)
    nv, nt = mesh.nv, mesh.nt
    assert nv > 10 and nt > 10
    assert mesh.run(ctx, iso, above, 0, 0, outputs=False) == (0, nv, nt) and mesh.untouched()    # count only
    for vertex_capacity, triangle_capacity, counted, given in ((nv - 1, nt, nv, nv - 1), (nv, nt - 1, nt, nt - 1)):
        assert mesh.run(ctx, iso, above, vertex_capacity, triangle_capacity) == (1, nv, nt)
        assert str(counted) in capi.last_error() and str(given) in capi.last_error()
        assert mesh.untouched()
    assert mesh.run(ctx, iso, above, nv, nt) == (0, nv, nt)                                     # exact capacity
    assert _same(mesh.mesh(), want) and mesh.untouched(nv, nt)
    first = [t.clone() for t in (mesh.vertices, mesh.triangles, mesh.cells)]
    for t in (mesh.vertices, mesh.triangles, mesh.cells):
        t.fill_(SENTINEL)
    assert mesh.run(ctx, iso, above, nv + 5, nt + 5) == (0, nv, nt)
    assert all(torch.equal(a, b) for a, b in zip(first, (mesh.vertices, mesh.triangles, mesh.cells)))  # equal bytes
    # the host form: one short on either list fails and leaves the caller's arrays as they were
    vertices = np.full((nv, 3), 7.0)
    triangles = np.full((nt, 3), 7, np.int32)
    count = [ctypes.c_int64(-1), ctypes.c_int64(-1)]
    for vertex_capacity, triangle_capacity in ((nv - 1, nt), (nv, nt - 1)):
        rc = ctx._lib.vgt_hip_extract_surface(ctx.handle, capi._ptr(values), *values.shape, iso, int(above), 0.25, None,
                                              capi._ptr(vertices), None, vertex_capacity, capi._ptr(triangles),
                                              triangle_capacity, ctypes.byref(count[0]), ctypes.byref(count[1]))
        assert rc == 1 and (count[0].value, count[1].value) == (nv, nt)
        assert (vertices == 7.0).all() and (triangles == 7).all()
    with pytest.raises(ValueError):
        capi.check(rc)


LAYOUTS = [(None, -1), (capi.OCCUPANCY_COMPONENT_CELL, -1), (capi.TAGGED_OBJECT_CELL, 4),
           (capi.TAGGED_OBJECT_COMPONENT_CELL, 4)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=["float4", "component8", "tagged8", "tagged16"])
def test_cells_entry_point(ctx, layout):
    dtype, id_offset = layout
    shape = (4, 5, 65)
    occupancy, iso, above, want = _reference("occupancy", shape)
    assert (iso, above) == (0.5, True)
    if dtype is None:
        records = occupancy
    else:
        rng = np.random.default_rng(3)
        records = np.zeros(shape, dtype=dtype)
        records["occupancy"] = occupancy
        for name in dtype.names[1:]:
            records[name] = rng.integers(0, 1 << 32, size=shape, dtype=np.uint32)
    cells = ctx.cells(records, shape, object_id_offset=id_offset)
    try:
        assert _same(cells.extract_surface(0.25, with_cells=True), want)
        assert _same(ctx.extract_surface(occupancy, 0.25, 0.5, True, with_cells=True), want)
        transformed = _reference("occupancy", shape, 0.25, True)[3]
        assert _same(cells.extract_surface(0.25, C.rotation_and_translation()), transformed[:2])
    finally:
        cells.close()


def test_dev_on_the_callers_stream(ctx, torch):
    values, iso, above, want = _reference("noise", (17, 9, 70))
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        field = torch.from_numpy(values.copy()).cuda()
    stream.synchronize()
    ctx.set_stream(stream.cuda_stream)
    try:
        first = ctx.extract_surface_dev(field, 0.25, iso, above, with_cells=True)
        second = ctx.extract_surface_dev(field.data_ptr(), 0.25, iso, above, with_cells=True, shape=values.shape)
    finally:
        ctx.reset_stream()
    assert all(t.is_cuda for t in first) and first[0].dtype == torch.float64 and first[1].dtype == torch.int32
    assert _same(first, want) and _same(second, want)
    assert _same(ctx.extract_surface(values, 0.25, iso, above, with_cells=True), want)          # the host form


@pytest.mark.parametrize("kind", sorted(C.SOLIDS))
def test_closed_surfaces_of_the_library_sdf(ctx, torch, kind):
    filled = C.solid(kind, 64)
    resolution = 0.05
    sdf, lo, hi = ctx.sdf_from_occupancy(filled.astype(np.float32), resolution)
    assert lo < 0 < hi
    vertices, triangles = (t.cpu().numpy() for t in ctx.extract_surface_dev(torch.from_numpy(sdf).cuda(), resolution))
    quads = R.quads_of(triangles)
    assert R.is_closed_manifold(quads)
    assert R.euler_characteristic(len(vertices), quads) == C.SOLIDS[kind]
    volume = R.signed_volume(vertices, triangles)
    assert volume > 0
    print(kind, "volume error in cells", abs(volume / resolution ** 3 - filled.sum()), "active cubes", len(vertices))
    assert abs(volume - filled.sum() * resolution ** 3) <= len(vertices) * resolution ** 3


def test_mesh_to_sdf_to_mesh_to_map_on_the_device(ctx, torch):
    """Formats only: what extract_surface_dev leaves on the device is what rasterize_mesh_dev takes."""
    v, t = synthetic.mesh_icosphere(1, radius=0.4)
    resolution = 0.05
    sdf, lo, hi, _ = ctx.mesh_sdf(v, t, resolution, rule=capi.MESH_RULE_NEAREST, solid=True)
    assert lo < 0 < hi
    vertices, triangles = ctx.extract_surface_dev(torch.from_numpy(sdf).cuda(), resolution)
    assert len(vertices) > 0 and len(triangles) > 0
    fresh = torch.zeros(sdf.shape, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.rasterize_mesh_dev(vertices.data_ptr(), len(vertices), triangles.data_ptr(), len(triangles), fresh.data_ptr(), 4,
                           sdf.shape, resolution, rule=capi.MESH_RULE_NEAREST)
    ctx.synchronize()
    assert int((fresh == 1.0).sum()) >= 1
