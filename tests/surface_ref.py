"""numpy restatement of vgt_hip_extract_surface (include/vgt_hip.h): surface nets on the lattice of cell centres.

Two forms that must give equal bytes: extract_loop, a literal triple loop in Python floats (IEEE double, one operation
at a time), and extract, vectorised, for the larger cases.  Both add the crossing edges' offsets in the stated edge order
and apply the transform left to right; numpy's elementwise double arithmetic contracts nothing.

Also the checks the tests share: closure, Euler characteristic and signed volume of a quad mesh.
"""
import numpy as np


def _inside(values, iso, inside_above):
    with np.errstate(invalid="ignore"):
        return values > iso if inside_above else values < iso


def _transform(m, x, y, z):
    """Row r of a column-major 4 x 4: M[r] * x + M[4 + r] * y + M[8 + r] * z + M[12 + r], left to right."""
    return [m[r] * x + m[4 + r] * y + m[8 + r] * z + m[12 + r] for r in range(3)]


def extract_loop(values, resolution, iso=0.0, inside_above=False, world_from_grid=None):
    """-> (vertices float64 [V, 3], triangles int32 [T, 3], cells int32 [V]), the definition read aloud."""
    f = np.ascontiguousarray(values, dtype=np.float32)
    nx, ny, nz = f.shape
    iso32 = np.float32(iso)
    res = float(resolution)
    m = None if world_from_grid is None else [float(v) for v in np.asarray(world_from_grid, dtype=np.float64).reshape(16)]

    def inside(v):
        return bool(v > iso32) if inside_above else bool(v < iso32)

    vertex_of = {}
    vertices, cells = [], []
    for i in range(nx - 1):
        for j in range(ny - 1):
            for k in range(nz - 1):
                corners = f[i:i + 2, j:j + 2, k:k + 2]
                if not np.isfinite(corners).all():
                    continue
                flags = [inside(v) for v in corners.ravel()]
                if all(flags) or not any(flags):
                    continue
                offset = [0.0, 0.0, 0.0]
                n = 0
                for a in range(3):
                    b, c = (a + 1) % 3, (a + 2) % 3
                    for db, dc in ((0, 0), (0, 1), (1, 0), (1, 1)):
                        p0 = [0, 0, 0]
                        p0[b], p0[c] = db, dc
                        p1 = list(p0)
                        p1[a] = 1
                        v0, v1 = corners[tuple(p0)], corners[tuple(p1)]
                        if inside(v0) != inside(v1):
                            t = (float(iso32) - float(v0)) / (float(v1) - float(v0))
                            offset[a] += t
                            offset[b] += float(db)
                            offset[c] += float(dc)
                            n += 1
                location = [((float(index) + 0.5) + offset[axis] / float(n)) * res
                            for axis, index in enumerate((i, j, k))]
                if m is not None:
                    location = _transform(m, *location)
                cell = (i * ny + j) * nz + k
                vertex_of[cell] = len(vertices)
                vertices.append(location)
                cells.append(cell)
    extents = (nx, ny, nz)
    strides = (ny * nz, nz, 1)
    triangles = []
    for i in range(nx):
        for j in range(ny):
            for k in range(nz):
                p = (i, j, k)
                linear = (i * ny + j) * nz + k
                for a in range(3):
                    b, c = (a + 1) % 3, (a + 2) % 3
                    if p[a] + 1 >= extents[a] or p[b] < 1 or p[c] < 1:
                        continue
                    q = list(p)
                    q[a] += 1
                    if inside(f[p]) == inside(f[tuple(q)]):
                        continue
                    c00, c10, c11, c01 = linear - strides[b] - strides[c], linear - strides[c], linear, linear - strides[b]
                    if not all(cube in vertex_of for cube in (c00, c10, c11, c01)):
                        continue
                    loop = (c00, c10, c11, c01) if inside(f[p]) else (c00, c01, c11, c10)
                    q0, q1, q2, q3 = (vertex_of[cube] for cube in loop)
                    triangles.append((q0, q1, q2))
                    triangles.append((q0, q2, q3))
    return (np.array(vertices, dtype=np.float64).reshape(-1, 3), np.array(triangles, dtype=np.int32).reshape(-1, 3),
            np.array(cells, dtype=np.int32))


def extract(values, resolution, iso=0.0, inside_above=False, world_from_grid=None):
    """The same, vectorised -> (vertices, triangles, cells)."""
    f = np.ascontiguousarray(values, dtype=np.float32)
    nx, ny, nz = f.shape
    iso32 = np.float32(iso)
    res = np.float64(resolution)
    if min(nx, ny, nz) < 2:
        return np.zeros((0, 3), np.float64), np.zeros((0, 3), np.int32), np.zeros(0, np.int32)
    ins = _inside(f, iso32, inside_above)
    fin = np.isfinite(f)

    def corner(array, d):
        return array[d[0]:nx - 1 + d[0], d[1]:ny - 1 + d[1], d[2]:nz - 1 + d[2]]

    all_corners = [(a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)]
    finite = np.logical_and.reduce([corner(fin, d) for d in all_corners])
    count = sum(corner(ins, d).astype(np.int32) for d in all_corners)
    cube_active = finite & (count > 0) & (count < 8)
    offset = [np.zeros(cube_active.shape, np.float64) for _ in range(3)]
    n = np.zeros(cube_active.shape, np.float64)
    with np.errstate(all="ignore"):
        for a in range(3):
            b, c = (a + 1) % 3, (a + 2) % 3
            for db, dc in ((0, 0), (0, 1), (1, 0), (1, 1)):
                p0 = [0, 0, 0]
                p0[b], p0[c] = db, dc
                p1 = list(p0)
                p1[a] = 1
                v0, v1 = corner(f, p0).astype(np.float64), corner(f, p1).astype(np.float64)
                cross = corner(ins, p0) != corner(ins, p1)
                t = (np.float64(iso32) - v0) / (v1 - v0)
                # (+ 0.0 leaves a sum that started at + 0.0 as it is: the skipped edges of the loop form)
                offset[a] = offset[a] + np.where(cross, t, 0.0)
                offset[b] = offset[b] + np.where(cross, np.float64(db), 0.0)
                offset[c] = offset[c] + np.where(cross, np.float64(dc), 0.0)
                n = n + cross
        index = np.meshgrid(np.arange(nx - 1, dtype=np.float64), np.arange(ny - 1, dtype=np.float64),
                            np.arange(nz - 1, dtype=np.float64), indexing="ij")
        location = [((index[axis] + 0.5) + offset[axis] / n) * res for axis in range(3)]
        if world_from_grid is not None:
            location = _transform(np.asarray(world_from_grid, dtype=np.float64).reshape(16), *location)
    active = np.zeros(f.shape, dtype=bool)  # by the cube's lowest corner, in the sample grid
    active[:nx - 1, :ny - 1, :nz - 1] = cube_active
    flat_active = active.ravel()
    cells = np.flatnonzero(flat_active).astype(np.int32)
    vertices = np.stack([axis[cube_active] for axis in location], axis=1).reshape(-1, 3)
    vertex_of = np.cumsum(flat_active) - 1

    extents = (nx, ny, nz)
    strides = (ny * nz, nz, 1)
    coords = np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij")
    linear = np.arange(nx * ny * nz).reshape(f.shape)
    faces = np.zeros(f.shape + (3,), dtype=bool)
    quads = np.zeros(f.shape + (3, 4), dtype=np.int64)
    for a in range(3):
        b, c = (a + 1) % 3, (a + 2) % 3
        ok = (coords[a] + 1 < extents[a]) & (coords[b] >= 1) & (coords[c] >= 1)
        cross = ok & (ins != np.roll(ins, -1, axis=a))
        cubes = [linear - strides[b] - strides[c], linear - strides[c], linear, linear - strides[b]]  # c00 c10 c11 c01
        for cube in cubes:
            cross &= flat_active[np.where(ok, cube, 0)]
        faces[..., a] = cross
        plus = ins  # p inside: the normal is + a
        quads[..., a, 0] = cubes[0]
        quads[..., a, 1] = np.where(plus, cubes[1], cubes[3])
        quads[..., a, 2] = cubes[2]
        quads[..., a, 3] = np.where(plus, cubes[3], cubes[1])
    q = vertex_of[quads[faces]]  # ascending p, then axis
    triangles = np.stack([q[:, [0, 1, 2]], q[:, [0, 2, 3]]], axis=1).reshape(-1, 3).astype(np.int32)
    return vertices, triangles, cells


def quads_of(triangles):
    """The quads (q0, q1, q2, q3) of a triangle list that holds (q0, q1, q2), (q0, q2, q3) per quad."""
    t = np.asarray(triangles).reshape(-1, 2, 3)
    assert np.array_equal(t[:, 0, 0], t[:, 1, 0]) and np.array_equal(t[:, 0, 2], t[:, 1, 1])
    return np.stack([t[:, 0, 0], t[:, 0, 1], t[:, 0, 2], t[:, 1, 2]], axis=1).astype(np.int64)


def directed_edge_counts(quads):
    """{(from, to): how often} over the four sides of every quad."""
    q = np.asarray(quads)
    edges = np.concatenate([np.stack([q[:, s], q[:, (s + 1) % 4]], axis=1) for s in range(4)])
    unique, counts = np.unique(edges, axis=0, return_counts=True)
    return {(int(a), int(b)): int(n) for (a, b), n in zip(unique, counts)}


def is_closed(quads):
    """Per directed edge, the count equals the count of its reverse (holds for non-manifold closed meshes too)."""
    edges = directed_edge_counts(quads)
    return all(edges.get((b, a), 0) == n for (a, b), n in edges.items())


def is_closed_manifold(quads):
    """Every directed edge occurs once and its reverse exactly once."""
    edges = directed_edge_counts(quads)
    return all(n == 1 and edges.get((b, a), 0) == 1 for (a, b), n in edges.items())


def euler_characteristic(num_vertices, quads):
    edges = directed_edge_counts(quads)
    undirected = {(min(a, b), max(a, b)) for a, b in edges}
    return num_vertices - len(undirected) + len(quads)


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(triangles)
    return float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)
