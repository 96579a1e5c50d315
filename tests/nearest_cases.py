"""Inputs of the nearest-other-class tests (tests/test_gpu_nearest.py): the smallest grids at which each mechanism of
csrc/nearest_kernels.hip can go wrong.  Plain numpy; every case is (name, float32 occupancy, unknown_is_filled)."""
import numpy as np

from voxelized_geometry_tools_amd import synthetic


def filled_of(occupancy, unknown_is_filled=True):
    """The predicate of vgt_hip_sdf_dev: > 0.5, or == 0.5 with unknown_is_filled (NaN is free)."""
    occ = np.asarray(occupancy, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (occ > np.float32(0.5)) | (bool(unknown_is_filled) & (occ == np.float32(0.5)))


def _grid(shape, cells=(), background=0.0, value=1.0):
    occ = np.full(shape, background, dtype=np.float32)
    for c in cells:
        occ[c] = value
    return occ


def _seeded(shape, fill, seed):
    rng = np.random.RandomState(seed)
    return (rng.random_sample(shape) < fill).astype(np.float32)


def _seeded_sites(shape, count, seed):
    rng = np.random.RandomState(seed)
    occ = np.zeros(shape, dtype=np.float32)
    for _ in range(count):
        occ[tuple(rng.randint(0, s) for s in shape)] = 1.0
    return occ


def cases():
    out = []

    def add(name, occ, unknown_is_filled=True):
        out.append((name, np.ascontiguousarray(occ, dtype=np.float32), unknown_is_filled))

    add("1x1x1 filled", _grid((1, 1, 1), background=1.0))
    add("1x1x1 free", _grid((1, 1, 1)))
    add("3x2x5 one filled corner", _grid((3, 2, 5), [(0, 0, 0)]))
    add("3x2x5 one free cell", _grid((3, 2, 5), [(1, 1, 2)], background=1.0, value=0.0))
    add("3x2x5 all free", _grid((3, 2, 5)))
    add("3x2x5 all filled", _grid((3, 2, 5), background=1.0))
    # Z lines across the edges of the 64-cell class words
    for n in (2, 63, 64, 65, 129):
        add("z line %d, sites at both ends" % n, _grid((1, 1, n), [(0, 0, 0), (0, 0, n - 1)]))
        add("z line %d, a site in the last word only" % n, _grid((1, 1, n), [(0, 0, n - 1 - (n > 2) * ((n - 1) % 64 // 2))]))
    # partial waves of the line passes
    for nz in (1, 63, 65):
        add("3x3x%d seeded" % nz, _seeded((3, 3, nz), 0.3, 100 + nz))
    # every cell ties
    x, y, z = np.indices((9, 9, 9))
    add("2x2x2 checkerboard", (np.indices((2, 2, 2)).sum(axis=0) % 2).astype(np.float32))
    add("9x9x9 checkerboard", ((x + y + z) % 2).astype(np.float32))
    planes = np.zeros((9, 4, 5), dtype=np.float32)
    planes[0] = planes[8] = 1.0
    add("two filled planes x = 0 and x = 8", planes)
    # deep stacks: along x the heights (z - x')^2 of the wall keep the sites on the hull, the filled cells' envelope
    # holds all 300 rows; the plane gives every row of an X line the same height
    wall = np.zeros((300, 2, 300), dtype=np.float32)
    i = np.arange(300)
    wall[i, :, i] = 1.0
    add("diagonal wall 300x2x300", wall)
    plane = np.zeros((300, 2, 3), dtype=np.float32)
    plane[:, 0, :] = 1.0
    add("filled plane y = 0 at 300x2x3", plane)
    for k, shape in enumerate(((2050, 3, 2), (2, 2050, 3), (3, 2, 2050))):
        add("%dx%dx%d, a dozen sites" % shape, _seeded_sites(shape, 12, 7 + k))
    for shape in ((16384, 1, 1), (1, 16384, 1), (1, 1, 16384)):
        add("%dx%dx%d, the site at index 0" % shape, _grid(shape, [(0, 0, 0)]))
    for fill in (0.001, 0.5, 0.999):
        add("70x33x130 seeded, fill %g" % fill, _seeded((70, 33, 130), fill, int(fill * 1000)))
    mix = synthetic.occupancy_unknown_mix((40, 36, 70), seed=5)
    add("unknown mix, unknown is filled", mix, True)
    add("unknown mix, unknown is free", mix, False)
    return out


def tagged_scene(shape=(24, 20, 18)):
    """(occupancy, object ids) of three box objects plus filled and unknown cells of object 0."""
    occ = np.zeros(shape, dtype=np.float32)
    ids = np.zeros(shape, dtype=np.uint32)
    boxes = {1: (slice(2, 7), slice(3, 9), slice(2, 6)), 2: (slice(12, 20), slice(2, 6), slice(8, 15)),
             3: (slice(8, 12), slice(12, 18), slice(4, 16))}
    for object_id, box in boxes.items():
        occ[box] = 1.0
        ids[box] = object_id
    occ[20:23, 15:19, 0:3] = 1.0      # filled, object 0
    occ[0:2, 0:2, 10:12] = 0.5        # unknown, object 0
    ids[5:9, 10:12, 8:10] = 2         # free cells that carry an id
    return occ, ids
