"""Inputs shared by tests/test_consumer_ref.py (CPU) and tests/test_gpu_consumers.py (GPU): fields, resolutions, frames
and query points at the edges of the four SDF consumers of csrc/cell_kernels.hip (coarse gradient, trilinear estimate,
fine gradient, local-extrema map).  tests/consumer_ref.py restates the operations.

Three kinds of case, each a namedtuple of read-only arrays built once:
  FieldCase    (name, field, resolution)                                   coarse gradient; the base of the others
  QueryCase    (name, field, resolution, grid_from_world, queries)         estimate
  FineCase     (name, field, resolution, grid_from_world, queries, window, raises, branch, axis)   fine gradient
  ExtremaCase  (name, field, resolution, rotation)                         local-extrema map
grid_from_world is 16 doubles column-major (InverseOriginTransform) or None for the grid frame; rotation is the 3x3
row-major rotation of the origin transform (world from grid) or None.
"""
import collections
import functools

import numpy as np

import consumer_ref as R

FieldCase = collections.namedtuple("FieldCase", "name field resolution")
QueryCase = collections.namedtuple("QueryCase", "name field resolution grid_from_world queries")
FineCase = collections.namedtuple("FineCase", "name field resolution grid_from_world queries window raises branch axis")
ExtremaCase = collections.namedtuple("ExtremaCase", "name field resolution rotation")

SHAPES = [(1, 1, 1), (1, 1, 5), (2, 2, 2), (1, 6, 5), (7, 1, 3), (9, 8, 10), (33, 3, 64)]
RESOLUTIONS = [0.125, 0.1, 1.0 / 3.0, 0.04]
FIELD_KINDS = ["plus_inf", "minus_inf", "non_finite", "signed_zero"]
TINY = np.float32(1e-45)                                        # the smallest float32 subnormal


def _frozen(a, dtype):
    a = np.ascontiguousarray(a, dtype=dtype)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def field(kind, shape):
    """One of FIELD_KINDS (or "normal") at a shape, float32, read-only."""
    rng = np.random.default_rng(1000 * FIELD_KINDS.index(kind) + sum((k + 1) * n for k, n in enumerate(shape))
                                if kind in FIELD_KINDS else sum((k + 3) * n for k, n in enumerate(shape)))
    total = int(np.prod(shape))
    if kind == "plus_inf":                                      # the library's own field of an empty map
        f = np.full(shape, np.inf, dtype=np.float32)
    elif kind == "minus_inf":                                   # ... and of a full one
        f = np.full(shape, -np.inf, dtype=np.float32)
    elif kind == "normal":
        f = rng.normal(size=shape).astype(np.float32)
    elif kind == "non_finite":
        # finite, with +inf, -inf and NaN once on a face and once in the interior (as far as the shape has such cells)
        f = rng.normal(size=shape).astype(np.float32)
        idx = np.indices(shape).reshape(3, -1)
        interior = np.ones(total, dtype=bool)
        for a in range(3):
            interior &= (idx[a] > 0) & (idx[a] < shape[a] - 1)
        flat = f.reshape(-1)
        for cells in (np.flatnonzero(~interior), np.flatnonzero(interior)):
            chosen = rng.permutation(cells)[:3]
            flat[chosen] = np.array([np.inf, -np.inf, np.nan], dtype=np.float32)[:len(chosen)]
    elif kind == "signed_zero":
        # +0.0, -0.0 and +-1e-45 among ordinary values: the zeros and subnormals sit next to differences that are not flat
        specials = np.array([0.0, -0.0, TINY, -TINY], dtype=np.float32)
        f = rng.normal(size=shape).astype(np.float32)
        flat = f.reshape(-1)
        pick = rng.random(total) < 0.5
        flat[pick] = specials[rng.integers(0, 4, size=int(pick.sum()))]
        first = rng.permutation(total)[:4]
        flat[first] = np.roll(specials, -1)[:len(first)]          # every special occurs (a single cell holds -0.0)
    else:
        raise KeyError(kind)
    return _frozen(f, np.float32)


# ---- frames ----
def _rigid(axis, angle, translation):
    """world_from_grid 4x4 (row-major numpy) of a rotation about `axis` and a translation."""
    axis = np.asarray(axis, dtype=np.float64)
    axis = axis / np.linalg.norm(axis)
    k = np.array([[0.0, -axis[2], axis[1]], [axis[2], 0.0, -axis[0]], [-axis[1], axis[0], 0.0]])
    rot = np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * (k @ k)
    m = np.eye(4)
    m[:3, :3] = rot
    m[:3, 3] = translation
    return m


def _quarter_turn():
    m = np.eye(4)
    m[:3, :3] = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]
    m[:3, 3] = [0.5, -0.25, 0.125]
    return m


def _translation():
    m = np.eye(4)
    m[:3, 3] = [0.4, -0.3, 0.25]
    return m


WORLD_FROM_GRID = collections.OrderedDict([
    ("grid", None), ("identity", np.eye(4)), ("translation", _translation()), ("quarter_turn", _quarter_turn()),
    ("rigid", _rigid((1.0, 2.0, 3.0), 0.7, (0.3, -0.2, 0.15)))])
FRAMES = list(WORLD_FROM_GRID)
ROTATED_FRAMES = ["quarter_turn", "rigid"]


def grid_from_world(frame):
    """16 doubles column-major, or None for the grid frame."""
    m = WORLD_FROM_GRID[frame]
    if m is None:
        return None
    if frame in ("identity", "quarter_turn"):                   # exact inverses of exact matrices
        inv = np.eye(4)
        inv[:3, :3] = m[:3, :3].T
        inv[:3, 3] = -(m[:3, :3].T @ m[:3, 3])
    else:
        inv = np.linalg.inv(m)
    return _frozen(inv.T.reshape(-1), np.float64)


def rotation(frame):
    """3x3 row-major rotation of the origin transform, or None."""
    m = WORLD_FROM_GRID[frame]
    return None if m is None else _frozen(m[:3, :3], np.float64)


def to_world(queries, frame):
    m = WORLD_FROM_GRID[frame]
    if m is None:
        return queries
    with np.errstate(all="ignore"):
        return queries @ m[:3, :3].T + m[:3, 3]


# ---- query points ----
def _axis_values(n, res):
    """Coordinates along one axis of n cells that decide floor(g * (1 / res)): every cell boundary k * res (the faces
    included) and its two neighbours in double, -0.0 and the smallest negative double."""
    values = []
    for k in range(n + 1):
        b = k * res
        values += [np.nextafter(b, -np.inf), b, np.nextafter(b, np.inf)]
    return values + [-0.0, -5e-324]


@functools.lru_cache(maxsize=None)
def grid_queries(shape, res):
    """Query points [N, 3] in the grid frame for a shape and a resolution (read-only)."""
    centres = [(np.arange(n, dtype=np.float64) + 0.5) * res for n in shape]   # as the kernel computes a centre
    q = [np.stack(np.meshgrid(*centres, indexing="ij"), axis=-1).reshape(-1, 3)]
    # lines through the boundaries of one axis, the other two at a cell centre and at two off-centre places
    for a in range(3):
        values = np.array(_axis_values(shape[a], res))
        for offset in (0.5, 0.25, 0.75):
            line = np.empty((len(values), 3))
            for b in range(3):
                line[:, b] = (shape[b] // 2 + offset) * res
            line[:, a] = values
            q.append(line)
    # the corners of the grid: both faces of every axis with their neighbours, all combinations
    face_values = []
    for n in shape:
        top = n * res
        face_values.append([np.nextafter(0.0, -np.inf), -0.0, 0.0, np.nextafter(0.0, np.inf), np.nextafter(top, -np.inf), top])
    q.append(np.stack(np.meshgrid(*face_values, indexing="ij"), axis=-1).reshape(-1, 3))
    q.append(non_finite_queries(shape, res))
    return _frozen(np.concatenate(q), np.float64)


def non_finite_queries(shape, res):
    mid = [(n // 2 + 0.25) * res for n in shape]
    out = []
    for a in range(3):
        for v in (np.nan, np.inf, -np.inf):
            p = list(mid)
            p[a] = v
            out.append(p)
    out += [[np.nan] * 3, [np.inf] * 3, [-np.inf] * 3]
    return np.array(out, dtype=np.float64)


def field_cases(kinds=FIELD_KINDS, shapes=SHAPES, resolutions=RESOLUTIONS):
    return [FieldCase("%s-%s-res%.4g" % (kind, "x".join(map(str, shape)), res), field(kind, shape), res)
            for kind in kinds for shape in shapes for res in resolutions]


def query_cases(kind, shape):
    """Every resolution and frame for one field: the grid-frame points carried into the frame's world, and for the
    frames with a transform also the non-finite coordinates themselves."""
    cases = []
    f = field(kind, shape)
    for res in RESOLUTIONS:
        base = grid_queries(shape, res)
        for frame in FRAMES:
            q = to_world(base, frame)
            if frame != "grid":
                q = np.concatenate([q, non_finite_queries(shape, res)])
            cases.append(QueryCase("%s-%s-res%.4g-%s" % (kind, "x".join(map(str, shape)), res, frame), f, res,
                                   grid_from_world(frame), _frozen(q, np.float64)))
    return cases


FIELD_AND_SHAPE = [(kind, shape) for kind in FIELD_KINDS for shape in SHAPES]


# ---- fine gradient ----
FINE_SHAPE, FINE_RES, FINE_WINDOW = (9, 8, 10), 0.125, 0.04
BRANCH_NAMES = {R.BRANCH_BOTH: "both", R.BRANCH_MINUS_ONLY: "minus_only", R.BRANCH_PLUS_ONLY: "plus_only"}


def _fine_candidates(shape, res, window, seed):
    """Grid-frame points all over the grid, a good part of them within a window of one face."""
    rng = np.random.default_rng(seed)
    extent = np.array(shape, dtype=np.float64) * res
    q = rng.random((6000, 3)) * extent
    near = rng.integers(0, 3, size=len(q))
    side = rng.integers(0, 3, size=len(q))                        # 0: leave, 1: lower face, 2: upper face
    depth = rng.random(len(q)) * window * 1.2
    rows = np.arange(len(q))
    q[rows[side == 1], near[side == 1]] = depth[side == 1]
    q[rows[side == 2], near[side == 2]] = extent[near[side == 2]] - depth[side == 2]
    return q


@functools.lru_cache(maxsize=None)
def fine_cases():
    """The fine-gradient sets.  The branch sets are chosen with the restatement: a query belongs to the set of
    (branch, axis) when ComputeAxisFineGradient takes that branch on that axis and the two-sided one on the others."""
    cases = []
    f = field("normal", FINE_SHAPE)
    for frame in ["grid"] + ROTATED_FRAMES:
        xf = grid_from_world(frame)
        q = to_world(_fine_candidates(FINE_SHAPE, FINE_RES, FINE_WINDOW, 21), frame)
        branches = R.fine_gradient_branches(f, FINE_RES, q, FINE_WINDOW, xf)
        both = branches == R.BRANCH_BOTH
        for axis in range(3):
            others = both[:, (axis + 1) % 3] & both[:, (axis + 2) % 3]
            for branch in (R.BRANCH_MINUS_ONLY, R.BRANCH_PLUS_ONLY, R.BRANCH_BOTH):
                chosen = q[(branches[:, axis] == branch) & others]
                cases.append(FineCase("%s-%s-axis%d" % (frame, BRANCH_NAMES[branch], axis), f, FINE_RES, xf,
                                      _frozen(chosen, np.float64), FINE_WINDOW, False, branch, axis))
        # (near an edge of the grid a step along an oblique world axis leaves on both sides: those throw, and are left out)
        throws = (branches == R.BRANCH_NONE).any(axis=1)
        cases.append(FineCase("%s-negative_window" % frame, f, FINE_RES, xf, _frozen(q[~throws], np.float64), -FINE_WINDOW,
                              False, None, None))
        # an axis thinner than the window: both neighbours of every point in the grid are outside
        thin_shape, thin_window = (6, 5, 1), 0.2
        thin = field("normal", thin_shape)
        inside = to_world((np.random.default_rng(5).random((64, 3)) * 0.98 + 0.01) * np.array(thin_shape) * FINE_RES, frame)
        cases.append(FineCase("%s-thin_axis" % frame, thin, FINE_RES, xf, _frozen(inside, np.float64), thin_window, True,
                              None, None))
        # two cells thick: the middle band throws, the outer bands are one-sided; one thrower among good queries
        slab_shape = (6, 5, 2)
        slab = field("normal", slab_shape)
        good = (np.random.default_rng(6).random((40, 3)) * 0.2 + 0.4) * np.array(slab_shape) * FINE_RES
        good[:, 2] = np.where(np.arange(40) % 2 == 0, 0.01, 0.24)
        bad = np.array([[0.4, 0.3, 0.125]])
        mixed = to_world(np.concatenate([good[:20], bad, good[20:]]), frame)
        cases.append(FineCase("%s-good_only" % frame, slab, FINE_RES, xf, _frozen(to_world(good, frame), np.float64),
                              thin_window, False, None, None))
        cases.append(FineCase("%s-one_thrower" % frame, slab, FINE_RES, xf, _frozen(mixed, np.float64), thin_window, True,
                              None, None))
        outside = to_world(np.concatenate([_fine_candidates(FINE_SHAPE, FINE_RES, FINE_WINDOW, 22)[:200]
                                           + np.array(FINE_SHAPE) * FINE_RES * [1.0, 0.0, 0.0],
                                           non_finite_queries(FINE_SHAPE, FINE_RES)]), frame)
        cases.append(FineCase("%s-outside_only" % frame, f, FINE_RES, xf, _frozen(outside, np.float64), FINE_WINDOW, False,
                              None, None))
    return cases


# ---- local-extrema map ----
THRESHOLD_RES = 0.5


def _floats_around(value):
    """The largest float32 whose double is <= value and the smallest one above it."""
    f = np.float32(value)
    below = f if float(f) <= value else np.nextafter(f, np.float32(-np.inf))
    above = np.nextafter(below, np.float32(np.inf))
    assert float(below) <= value < float(above)
    return below, above


def threshold_fields():
    """(5, 5, 5) fields of zeros at resolution 0.5 in which one neighbour of a target cell holds the float32 that puts the
    target's gradient component at the nearest representable value below (flat) or above (a move) resolution * 0.06125;
    the interior target (2, 2, 2) divides the float difference by 1.0, the face target (index 0 on the axis, 2 on the
    others) the double difference by 0.5.  -> [(name, field, target cell, axis, sign, moves)]"""
    step = THRESHOLD_RES * R.STEP_FACTOR
    out = []
    for axis in range(3):
        for where, scale in (("interior", 1.0), ("face", 0.5)):
            for sign in (1.0, -1.0):
                for k, side in enumerate(("below", "above")):
                    value = _floats_around(step * scale)[k]
                    f = np.zeros((5, 5, 5), dtype=np.float32)
                    target = [2, 2, 2]
                    neighbour = [2, 2, 2]
                    if where == "interior":
                        neighbour[axis] = 3 if sign > 0 else 1
                    else:
                        target[axis] = 0
                        neighbour[axis] = 1 if sign > 0 else 0
                        if sign < 0:
                            f[tuple(target)] = value                 # the low cell is the target itself (uphill: >= 0)
                    f[tuple(neighbour)] = value
                    out.append(("threshold-%s-axis%d-%s-%s" % (where, axis, "up" if sign > 0 else "down", side),
                                _frozen(f, np.float32), tuple(target), axis, sign, side == "above"))
    return out


RAMP_CELLS, RAMP_RES, RAMP_SLOPE = 4096, 0.125, np.float32(2.0 ** -6)


def ramp(end):
    """(1, 1, 4096) ramp z * 2^-6 (exact in float32; gradient 0.125 per axis step, far above the threshold).
    end = "flat": the last two cells are equal, so the last one is flat and every chain ends there;
    end = "two_cycle": the last cell lies between its two predecessors, so it and cell 4094 point at each other and every
    chain from below enters the cycle at cell 4094;  end = "off_grid": the plain ramp, every chain leaves the grid."""
    f = np.arange(RAMP_CELLS, dtype=np.float32) * RAMP_SLOPE
    if end == "flat":
        f[-1] = f[-2]
    elif end == "two_cycle":
        f[-1] = f[-2] - RAMP_SLOPE * np.float32(0.5)
    else:
        assert end == "off_grid"
    return _frozen(f.reshape(1, 1, RAMP_CELLS), np.float32)


# A ring of four cells in a (1, 6, 6) slice at resolution 1, in (y, z): (0,2) -> (0,3) -> (1,3) -> (1,2) -> (0,2), cells
# 2, 3, 9 and 8.  Each ring cell's moving component is a difference of its neighbours, not of itself, which is how a
# cycle of more than two cells comes about at all.  Cells 0 and 1 leave the grid (cell 1 is negative and goes down and
# out), so cell 2, on the ring, is the smallest cell of the ring's basin: the first walk starts on the cycle.
RING_SLICE = np.array([
    [0.0, -1.0, 1.0, 1.0, 1.0, 0.0],
    [0.0, 2.0, 1.0, 2.0, 0.0, 0.0],
    [0.0, 0.0, 0.0, 1.0, 0.0, 0.0],
    [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
    [0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
    [0.0, 0.0, 0.0, 0.0, 0.0, 0.0]], dtype=np.float32)
RING_CELLS = [2, 3, 9, 8]
RING_RES = 1.0


def ring_field():
    return _frozen(RING_SLICE.reshape(1, 6, 6), np.float32)


def noise_field():
    """The 17 x 13 x 21 noise field of tests/test_gpu_gradient.py: full of cycles."""
    return _frozen(np.random.default_rng(7).normal(size=(17, 13, 21)), np.float32)


@functools.lru_cache(maxsize=None)
def extrema_cases():
    cases = []
    for kind in FIELD_KINDS:
        for shape in SHAPES:
            for res in (0.125, 0.1):
                for frame in ("grid", "rigid"):
                    cases.append(ExtremaCase("%s-%s-res%.4g-%s" % (kind, "x".join(map(str, shape)), res, frame),
                                             field(kind, shape), res, rotation(frame)))
    for name, f, _, _, _, _ in threshold_fields():
        cases.append(ExtremaCase(name, f, THRESHOLD_RES, None))
    for end in ("flat", "two_cycle", "off_grid"):
        cases.append(ExtremaCase("ramp-" + end, ramp(end), RAMP_RES, None))
    cases.append(ExtremaCase("ring", ring_field(), RING_RES, None))
    for shape in ((5, 1, 1), (1, 1, 1), (2, 2, 2)):
        for frame in ("grid", "quarter_turn"):
            cases.append(ExtremaCase("normal-%s-%s" % ("x".join(map(str, shape)), frame), field("normal", shape), 0.1,
                                     rotation(frame)))
    cases.append(ExtremaCase("noise", noise_field(), 0.1, None))
    return cases


CYCLE_CASES = ["noise", "ramp-two_cycle", "ring"]


def extrema_case(name):
    return next(c for c in extrema_cases() if c.name == name)


# ---- the stride-loop field ----
STRIDE_SHAPE = (16384, 33, 32)


def stride_field():
    """Cheap synthetic values for the one field larger than the kernels' 65536 x 256 threads: a hash of the cell index
    in [0, 1), so that neighbours differ everywhere."""
    i = np.arange(int(np.prod(STRIDE_SHAPE)), dtype=np.uint32)
    return ((i * np.uint32(2654435761)) >> np.uint32(8)).astype(np.float32).reshape(STRIDE_SHAPE) * np.float32(2.0 ** -24)
