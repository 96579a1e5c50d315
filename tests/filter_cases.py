"""Inputs shared by tests/test_filter_ref.py (CPU) and tests/test_gpu_filter.py (GPU): tracking counts, static occupancies
and filter options at the edges of the combine-and-filter rule (tests/filter_ref.py), the clouds and grids of the
share-accumulation tests, and the helper that writes counts into a tracking-grid handle's device memory.

A case is (tracking int32 [grids, cells, 2], static float32 [cells], options); an option is (percent_seen_free,
outlier_points_threshold, num_cameras_seen_free).  Families return lists of cases; every array is built once and
read-only.  tests/test_filter_ref.py shows that each family reaches all three outputs and a skipped cell, and that the
tie family tells the float rule from the double rule and `>=` from `>`.
"""
import collections
import functools

import numpy as np

Case = collections.namedtuple("Case", "name tracking static options")

_F = float.fromhex

# (seen free, seen filled, percent_seen_free), found by a search over the restatement and kept as literals.
# The float rule says free, the double rule filled: the threshold is one double-ulp above the exact ratio and rounds to
# the float ratio (an exact tie in float); in the last one both float conversions round down to 2^25 at the default 1.0.
FLOAT_FREE_DOUBLE_FILLED = [
    (3, 2, _F("0x1.3333333333334p-1")), (6, 4, _F("0x1.3333333333334p-1")), (9, 6, _F("0x1.3333333333334p-1")),
    (12, 8, _F("0x1.3333333333334p-1")), (1, 1, _F("0x1.0000000000001p-1")), (7, 7, _F("0x1.0000000000001p-1")),
    (1, 2, _F("0x1.5555555555556p-2")), (5, 10, _F("0x1.5555555555556p-2")), (3, 1, _F("0x1.8000000000001p-1")),
    (12, 4, _F("0x1.8000000000001p-1")), (1, 12, _F("0x1.3b13b13b13b15p-4")), (11, 1, _F("0x1.d555555555556p-1")),
    (2 ** 25 + 1, 1, 1.0),
]
# The float rule says filled, the double rule free: a count above 2^24 rounds in the float conversion; the threshold is
# the exact double ratio (an exact tie in double).
FLOAT_FILLED_DOUBLE_FREE = [
    (2 ** 24 + 1, 1, _F("0x1.fffffe0000040p-1")), (2 ** 24 + 1, 2, _F("0x1.fffffc00000c0p-1")),
    (2 ** 24 - 1, 4, _F("0x1.fffff80000180p-1")), (2 ** 24, 2 ** 24 + 3, _F("0x1.fffffd0000048p-2")),
    (2 ** 25 + 1, 5, _F("0x1.fffffb00000f0p-1")), (2, 2 ** 24 + 1, _F("0x1.fffffa0000120p-24")),
    (2 ** 24 + 1, 2 ** 26 + 5, _F("0x1.99999947ae14ep-3")), (2 ** 24, 2 ** 29 + 33, _F("0x1.f07c1d1745d36p-6")),
    (8, 2 ** 24 - 1, _F("0x1.fffff20000620p-22")), (2 ** 25 + 1, 2 ** 29 + 33, _F("0x1.e1e1e0f0f0f1ep-5")),
]
# Exact ties in both precisions: the ratio is the threshold.
TIES_IN_BOTH = [(3, 2, 0.6), (1, 1, 0.5), (12, 12, 0.5), (1, 3, 0.25), (2, 3, 0.4), (1, 2, 1.0 / 3.0), (4, 3, 4.0 / 7.0)]

LARGE_COUNTS = [1, 2 ** 24 - 1, 2 ** 24, 2 ** 24 + 1, 2 ** 29, 2 ** 30 - 1]
OUTLIER_THRESHOLDS = [1, 2, 7]
CAMERA_GRIDS = [1, 2, 5, 8]


# Static occupancies around the `<= 0.5` rule, as bit patterns so that no conversion can touch a NaN's payload:
# (float32 bits, skipped by the filter).
STATIC_BITS = [
    (0x3f000001, True),                                                    # nextafter(0.5, 1)
    (0x3f000000, False), (0x3effffff, False), (0x80000000, False),         # 0.5, nextafter(0.5, 0), -0.0
    (0x00000001, False), (0xbf800000, False), (0xff800000, False),         # smallest subnormal, -1, -inf
    (0x00000000, False),                                                   # 0
    (0x3f400000, True), (0x40000000, True), (0x7f800000, True), (0x3f800000, True),   # 0.75, 2, +inf, 1
    (0x7fc00000, True), (0xffc00000, True), (0x7f800001, True), (0x7fffffff, True),   # NaN: quiet, negative, signalling, all ones
]


def static_values():
    return np.array([b for b, _ in STATIC_BITS], dtype=np.uint32).view(np.float32)


def _case(name, tracking, static, options):
    tracking = np.ascontiguousarray(tracking, dtype=np.int32)
    static = np.ascontiguousarray(static, dtype=np.float32)
    assert tracking.ndim == 3 and tracking.shape[1:] == (static.size, 2)
    assert int(tracking.max()) < 2 ** 30 and int(tracking.min()) >= 0
    tracking.setflags(write=False)
    static.setflags(write=False)
    return Case(name, tracking, static, tuple(options))


def _one_grid(pairs):
    """One camera; a cell per (free, filled) pair, then an unseen cell and a skipped cell that has counts."""
    pairs = list(pairs) + [(0, 0), (5, 5)]
    occ = np.full(len(pairs), 0.5, dtype=np.float32)
    occ[-1] = np.float32(0.75)
    return np.array(pairs, dtype=np.int32)[None], occ


def tie_triples():
    return FLOAT_FREE_DOUBLE_FILLED + FLOAT_FILLED_DOUBLE_FREE + TIES_IN_BOTH


@functools.lru_cache(maxsize=None)
def ties():
    """Every committed triple's counts in one grid, filtered once per distinct threshold of the triples."""
    triples = tie_triples()
    tracking, occ = _one_grid([(a, b) for a, b, _ in triples])
    percents = sorted({p for _, _, p in triples})
    return [_case("ties", tracking, occ, [(p, 1, 1) for p in percents])]


def small_ratios():
    """Every distinct a / (a + b), 1 <= a, b <= 12, as the double quotient."""
    return sorted({a / (a + b) for a in range(1, 13) for b in range(1, 13)})


@functools.lru_cache(maxsize=None)
def ratio_sweep():
    """All count pairs 0 <= a, b <= 12 against every reachable ratio and the doubles on either side of it."""
    tracking, occ = _one_grid([(a, b) for a in range(13) for b in range(13)])
    options = []
    for r in small_ratios():
        options += [(float(np.nextafter(r, 0.0)), 1, 1), (r, 1, 1), (float(np.nextafter(r, 1.0)), 1, 1)]
    return [_case("ratio_sweep", tracking, occ, options)]


@functools.lru_cache(maxsize=None)
def large_counts():
    """Counts at and around 2^24, where the float conversion rounds, mixed over three cameras; a camera sees a cell with
    probability 1/2.  Outlier thresholds at 2^24 and 2^24 + 1 are compared as integers by the rule."""
    rng = np.random.default_rng(24)
    pairs = [(a, b) for a in LARGE_COUNTS for b in LARGE_COUNTS]
    cells = 12 * len(pairs)
    tracking = np.zeros((3, cells, 2), dtype=np.int32)
    for g in range(3):
        chosen = np.array(pairs, dtype=np.int32)[rng.integers(0, len(pairs), cells)]
        seen = rng.random(cells) < 0.5
        tracking[g] = chosen * seen[:, None]
    tracking[0, :len(pairs)] = pairs                     # every pair alone in one camera ...
    tracking[1:, :len(pairs)] = 0
    occ = np.full(cells, 0.5, dtype=np.float32)
    occ[::7] = np.float32(0.0)
    occ[5::31] = np.float32(1.0)                          # skipped
    options = [(1.0, 1, 1), (0.5, 1, 1), (float(np.nextafter(0.5, 1.0)), 1, 2), (_F("0x1.fffffe0000040p-1"), 1, 1),
               (float(np.float32(1.0) - np.float32(2.0 ** -24)), 2, 1), (2.0 ** -24, 2 ** 24, 1),
               (_F("0x1.fffffd0000048p-2"), 2 ** 24 + 1, 2), (2.0 ** -29, 2 ** 29, 3), (2.0 ** -6, 2 ** 30 - 1, 1)]
    return [_case("large_counts", tracking, occ, options)]


# The outlier family's cells: every (free, filled) of these in camera 0.
OUTLIER_FILLED = sorted({t + d for t in OUTLIER_THRESHOLDS for d in (-1, 0, 1)})      # 0 1 2 3 6 7 8
OUTLIER_FREE = [0, 1, 5]


@functools.lru_cache(maxsize=None)
def outlier():
    """Filled counts of t - 1, t and t + 1 for every threshold t on the same cells, with and without free counts: a
    cell whose only evidence is an outlier-zeroed filled count stays unknown, and becomes free once free > 0."""
    pairs = [(a, b) for a in OUTLIER_FREE for b in OUTLIER_FILLED]
    tracking, occ = _one_grid(pairs + pairs)
    tracking = np.concatenate([tracking, np.zeros_like(tracking)])       # a second camera that saw nothing ...
    tracking[1, len(pairs):2 * len(pairs), 0] = 2                        # ... and, on the second copy of the cells, free
    options = [(p, t, n) for t in OUTLIER_THRESHOLDS for p in (1.0, 0.5, 0.25) for n in (1, 2)]
    return [_case("outlier", tracking, occ, options)]


def outlier_cell(free, filled):
    """Index of the (free, filled) cell of outlier() whose second camera saw nothing."""
    return OUTLIER_FREE.index(free) * len(OUTLIER_FILLED) + OUTLIER_FILLED.index(filled)


@functools.lru_cache(maxsize=None)
def camera():
    """k of the G cameras see a cell free, k = 0 .. G, whichever camera comes first; one camera sees it filled while all
    the others see it free; ratios on either side of 0.6.  num_cameras_seen_free below, at and above G."""
    cases = []
    for grids in CAMERA_GRIDS:
        columns = []
        for k in range(grids + 1):
            for first in range(grids):
                column = np.zeros((grids, 2), dtype=np.int32)
                for j in range(k):
                    column[(first + j) % grids] = (3 + j, 0)
                columns.append(column)
        for filled_camera in range(grids):
            column = np.tile(np.array([[4, 0]], dtype=np.int32), (grids, 1))
            column[filled_camera] = (0, 1)
            columns.append(column)
            column = np.tile(np.array([[3, 2]], dtype=np.int32), (grids, 1))     # 0.6 exactly ...
            column[filled_camera] = (5, 4)                                      # ... and 0.556
            columns.append(column)
        columns.append(np.tile(np.array([[6, 0]], dtype=np.int32), (grids, 1)))  # the skipped cell
        tracking = np.stack(columns, axis=1)
        occ = np.full(len(columns), 0.5, dtype=np.float32)
        occ[1::3] = np.float32(0.0)
        occ[-1] = np.float32(1.0)
        options = [(p, 1, n) for n in (1, grids, grids + 1) for p in (1.0, 0.6, 0.5)]
        cases.append(_case("camera_%d" % grids, tracking, occ, options))
    return cases


def camera_free_cell(grids, k, first):
    """Cell of camera()'s case for `grids` cameras that k cameras, from camera `first` on, see free."""
    return k * grids + first


def camera_filled_cell(grids, filled_camera):
    """Cell of camera()'s case for `grids` cameras that one camera sees filled and all the others free."""
    return (grids + 1) * grids + 2 * filled_camera


STATIC_PATTERNS = [((0, 0), (0, 0)), ((3, 0), (0, 0)), ((0, 3), (2, 0)), ((3, 2), (3, 2)), ((0, 0), (1, 0))]


@functools.lru_cache(maxsize=None)
def static():
    """A row of static occupancies around 0.5 (and NaNs of four payloads) under every count pattern, two cameras."""
    values = static_values()
    occ = np.repeat(values, len(STATIC_PATTERNS))
    tracking = np.tile(np.array(STATIC_PATTERNS, dtype=np.int32).transpose(1, 0, 2), (1, len(values), 1))
    return [_case("static", tracking, occ, [(1.0, 1, 1), (0.6, 1, 2), (0.5, 3, 1)])]


def static_skipped():
    """bool per cell of static(): STATIC_BITS says the filter leaves it alone."""
    return np.repeat(np.array([s for _, s in STATIC_BITS], dtype=bool), len(STATIC_PATTERNS))


# FilterImpl hands the context's threads_per_block to LaunchFilter, which launches at most 256 * 64 workgroups.
FILTER_MAX_WORKGROUPS = 256 * 64
DEFAULT_THREADS = 256          # capi.Context() without a workgroup size
SMALLEST_THREADS = 64          # the smallest threads_per_block capi.Context accepts (a multiple of 64)


def over_the_cap(threads):
    return FILTER_MAX_WORKGROUPS * threads + 321


SMALL_SIZES = [1, 63, 255, 257, 4099]
SIZE_OPTIONS = [(_F("0x1.3333333333334p-1"), 2, 1), (_F("0x1.fffffe0000040p-1"), 1, 2)]


@functools.lru_cache(maxsize=1)
def mixture(cells):
    """`cells` cells of two cameras drawn from the other families' counts and static values.  The last cell and the first
    cell past the launch cap of either workgroup size (where the grid has one) are unknown cells that the filter changes
    under every option: a dropped tail or a loop that does not come round leaves them at 0.5."""
    rng = np.random.default_rng(cells)
    values = np.array([a for a, _, _ in tie_triples()] + [b for _, b, _ in tie_triples()] + LARGE_COUNTS +
                      OUTLIER_FILLED + list(range(13)), dtype=np.int32)
    tracking = values[rng.integers(0, len(values), (2, cells, 2))]
    tracking *= (rng.random((2, cells, 1)) < 0.6)
    tracking[1, :, 1] *= (rng.random(cells) < 0.3)
    statics = static_values()
    occ = statics[rng.integers(0, len(statics), cells)]
    occ[rng.random(cells) < 0.7] = np.float32(0.5)
    for n, cell in enumerate(marked_cells(cells)):
        occ[cell] = np.float32(0.5)
        tracking[:, cell] = ((0, 9), (0, 0)) if n % 2 == 0 else ((9, 0), (4, 0))
    return _case("mixture_%d" % cells, tracking, occ, SIZE_OPTIONS)


def marked_cells(cells):
    """The cells mixture() pins: the last one, and the first past each launch cap that the grid reaches."""
    return [cells - 1] + [c for c in (over_the_cap(DEFAULT_THREADS) - 321, over_the_cap(SMALLEST_THREADS) - 321)
                          if c < cells - 1]


def sizes():
    return [mixture(n) for n in SMALL_SIZES]


FAMILIES = collections.OrderedDict([("ties", ties), ("ratio_sweep", ratio_sweep), ("large_counts", large_counts),
                                    ("outlier", outlier), ("camera", camera), ("static", static), ("sizes", sizes)])


# ---- share accumulation: one cloud split over helper devices, the shares' grids summed into the caller's ----
ACCUMULATE_CAP_INTS = 256 * 32 * 256 * 4          # LaunchAccumulateCounts: 256 * 32 workgroups of 256 int4s
SPLIT_HELPERS = [[], [0], [0, 0, 0]]
SPLIT_GRIDS = [(1, 1, 1), (3, 3, 3), (5, 7, 9), (101, 3, 1), (162, 162, 162)]

Scene = collections.namedtuple("Scene", "counts points max_range xform voxel_size inverse_voxel_size sizes")


@functools.lru_cache(maxsize=1)
def split_scene(counts):
    """A cloud seen from inside the grid's last corner: every fourth point lies in the last voxel, so that each share of
    the cloud, whatever the split, counts in the grid's last ints; on the large grid the sensor sits three voxels from
    the far corner, where the flat index is beyond the accumulate kernel's launch cap."""
    from voxelized_geometry_tools_amd import synthetic
    large = int(np.prod(counts)) * 2 > ACCUMULATE_CAP_INTS
    vs = np.float32(0.05)
    ivs = np.float32(1.0) / vs
    sizes = tuple(np.float32(c) * vs for c in counts)
    npts = 3000 if large else 240
    rng = np.random.default_rng(int(np.prod(counts)))
    sensor = np.array([max(c - 3, 0) + 0.5 for c in counts]) * float(vs)
    pts = (rng.standard_normal((npts, 3)) * (0.4 if large else 0.15)).astype(np.float32)
    last_voxel = (np.array(counts) - 0.5) * float(vs)
    pts[::4] = (last_voxel - sensor + (rng.random((len(pts[::4]), 3)) - 0.5) * 0.02).astype(np.float32)
    pts[7::50] = np.float32(np.nan)
    xf = synthetic.translation_xform(*[float(s) for s in sensor]).astype(np.float32)
    pts.setflags(write=False)
    return Scene(tuple(counts), pts, 1.0, xf, vs, ivs, sizes)


def split_oracle(scene, points):
    from oracle import oracle as O
    return O.raycast_f32(points, scene.max_range, scene.xform, scene.voxel_size, scene.inverse_voxel_size, scene.sizes,
                         scene.counts)


@functools.lru_cache(maxsize=1)
def split_expected(counts):
    """(counts already in the grid, the oracle on the whole cloud, the oracle on the cloud's first 100 points, the oracle
    on the cloud's last quarter), each int32 [nx, ny, nz, 2] and read-only."""
    scene = split_scene(counts)
    before = np.random.default_rng(3).integers(1, 1000, scene.counts + (2,)).astype(np.int32)
    whole = split_oracle(scene, scene.points)
    again = split_oracle(scene, scene.points[:100])
    last_quarter = split_oracle(scene, scene.points[-(len(scene.points) // 4):])
    for a in (before, whole, again, last_quarter):
        a.setflags(write=False)
    return before, whole, again, last_quarter


# ---- device memory of a handle, written and read through the HIP runtime ----
def _hip():
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return hip, ctypes


def hip_memcpy_htod(dev_ptr, array):
    """Test helper: writes a host array into library-owned device memory via the HIP runtime."""
    hip, ctypes = _hip()
    a = np.ascontiguousarray(array)
    rc = hip.hipMemcpy(dev_ptr, a.ctypes.data_as(ctypes.c_void_p), a.nbytes, 1)
    assert rc == 0, "hipMemcpy failed: %d" % rc


def hip_memcpy_dtoh(dev_ptr, shape, dtype):
    """Test helper: reads library-owned device memory into a new host array via the HIP runtime."""
    hip, ctypes = _hip()
    out = np.empty(shape, dtype=dtype)
    rc = hip.hipMemcpy(out.ctypes.data_as(ctypes.c_void_p), dev_ptr, out.nbytes, 2)
    assert rc == 0, "hipMemcpy failed: %d" % rc
    return out
